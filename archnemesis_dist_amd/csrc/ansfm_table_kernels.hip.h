// ansfm_table_kernels.hip.h -- gfx950 kernels of ansfm_api.hip: layer and table preparation, the array-level calc_k seam,
// layer de-duplication, LBL tables and the layout helpers of the host-pointer seams.  The merge and RT kernels of the
// correlated-k hot path have units of their own (ansfm_overlap.hip, ansfm_overlapg.hip, ansfm_rt.hip).
//
// Data layout in HBM (all float64, "wave fastest" so that a wavefront = 64 consecutive
// wavenumbers reads/writes 512 contiguous bytes):
//   lnK    [NP][NT][S][G][Wpad]   ln k for k>0; k<=0 stored NaN-boxed (see encode_lnk)
//   tau    [n][L][G][Wpad]        vertical gas opacity per model/layer/g
//   cont   [n][L][Wpad]           continuum opacity (TAUCIA+TAUDUST+TAURAY), transposed on upload
// Wpad = W rounded up to 64; pad lanes carry k=0 and are never written back to the caller.
//
// Reference seams restated here (paths relative to the reference tree):
//   Spectroscopy_0.calc_k/calc_kg            Spectroscopy_0.py:2298-2437 / :2147-2295
//   ForwardModel_0.k_overlap / rank           ForwardModel_0.py:6029-6173
//   ForwardModel_0.calculate_layer_opacity    ForwardModel_0.py:3989, :4006
//   ForwardModel_0.calc_thermal_emission_spectrum / planck   ForwardModel_0.py:6287-6377 / :6183
//   ForwardModel_0.CIRSrad g-quadrature       ForwardModel_0.py:4504
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ansfm_merge_common.hip.h"

namespace ansfm {

__global__ void k_layer_prep(int n_layers_total, const double *__restrict__ lay_press_pa,
                             const double *__restrict__ lay_temp, int NP,
                             const double *__restrict__ PRESS, int NT,
                             const double *__restrict__ TEMP, double press_div, int grid_f32,
                             LayerInterp *__restrict__ out)
{
    // grid_f32: Spectroscopy_0.PRESS/TEMP are float32 arrays (tables read from .kta): NumPy then takes
    // np.log(PRESS[i]), phi-plo, thi-tlo and 1./(thi-tlo) in float32 (see include/ansfm.h, ansfm_set_f32_semantics)
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_layers_total) return;
    double press1 = lay_press_pa[i] / press_div;  // LayerX.PRESS/ATM_TO_PASCAL  ForwardModel_0.py:3855
    double temp1 = lay_temp[i];
    int ip = 0;
    double best = fabs(PRESS[0] - press1);
    for (int k = 1; k < NP; ++k) {
        double d = fabs(PRESS[k] - press1);
        if (d < best) { best = d; ip = k; }
    }
    int ipl, iph;
    bool pclamp = false;
    if (PRESS[ip] >= press1) {
        iph = ip;
        if (ip == 0) { press1 = PRESS[0]; ipl = 0; iph = 1; pclamp = true; }
        else ipl = ip - 1;
    } else {
        ipl = ip;
        if (ip == NP - 1) { press1 = PRESS[NP - 1]; iph = NP - 1; ipl = NP - 2; pclamp = true; }
        else iph = ip + 1;
    }
    int it = 0;
    best = fabs(TEMP[0] - temp1);
    for (int k = 1; k < NT; ++k) {
        double d = fabs(TEMP[k] - temp1);
        if (d < best) { best = d; it = k; }
    }
    int itl, ith;
    bool tclamp = false;
    if (TEMP[it] >= temp1) {
        ith = it;
        if (it == 0) { temp1 = TEMP[0]; itl = 0; ith = 1; tclamp = true; }
        else itl = it - 1;
    } else {
        itl = it;
        if (it == NT - 1) { temp1 = TEMP[NT - 1]; ith = NT - 1; itl = NT - 2; tclamp = true; }
        else ith = it + 1;
    }
    double lpress = log(press1), plo = log(PRESS[ipl]), phi = log(PRESS[iph]);
    double tlo = TEMP[itl], thi = TEMP[ith];
    double pden = phi - plo, tden = thi - tlo, dudt = 1. / tden;
    if (grid_f32) {
        plo = (double)(float)plo;
        phi = (double)(float)phi;
        if (pclamp) lpress = (double)(float)lpress;
        pden = (double)((float)phi - (float)plo);
        tden = (double)((float)thi - (float)tlo);
        dudt = (double)(1.0f / (float)tden);
    }
    LayerInterp r;
    r.ipl = ipl; r.iph = iph; r.itl = itl; r.ith = ith;
    r.v = (lpress - plo) / pden;
    r.u = (temp1 - tlo) / tden;
    if (grid_f32 && pclamp) r.v = (double)(((float)lpress - (float)plo) / (float)pden);   // all-float32 expression
    if (grid_f32 && tclamp) r.u = (double)(((float)temp1 - (float)tlo) / (float)tden);
    r.dudt = dudt;
    out[i] = r;
}

// ------------------------------------------------------------------------------------------------
// Table upload: K[W][G][NP][NT][S] (reference layout) -> lnK[NP][NT][S][G][Wpad].
// For every g this is a transpose between w and q = (p, t, s): 64 x 64 tiles through LDS, reads coalesced along q,
// writes coalesced along w.  k_table_check flags k < 0 / NaN or k decreasing in g (flag[0] |= 1) and any entry that
// encode_lnk boxes, k <= 0 or NaN (flag[0] |= 2), reading the source coalesced as well (one thread per (w, q), g sequential).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_table_relayout(const double *__restrict__ K, double *__restrict__ lnK, int W,
                                                        int Wpad, int G, int Q)
{
    __shared__ double tile[64][65];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;      // 64 x 4
    const int w0 = blockIdx.x * 64, q0 = blockIdx.y * 64, g = blockIdx.z;
    for (int r = ty; r < 64; r += 4) {
        const int w = w0 + r, q = q0 + tx;
        tile[r][tx] = (w < W && q < Q) ? K[((size_t)w * G + g) * Q + q] : 0.0;
    }
    __syncthreads();
    for (int r = ty; r < 64; r += 4) {
        const int q = q0 + r;
        if (q < Q) lnK[((size_t)q * G + g) * Wpad + w0 + tx] = encode_lnk(tile[tx][r]);      // pad lanes: k = 0
    }
}

// lnK[Q][G][Wpad] -> lnKg[Q][Wpad][Gs], Q = NP * NT * S and Gs = gfast_stride(G): the g-fastest copy that the forward merge's
// row-mapped lanes read (load_gas_rows).  The encoded doubles are copied as they are, so both copies agree by construction;
// the pad ordinate of an odd G gets the boxed 0 that the pad lanes (w >= W) already hold in lnK.  One block per (q, 64
// wavenumbers): reads coalesced along w, and the 64 * Gs doubles it writes are one contiguous run.  Grid (Q, Wpad / 64).
__global__ __launch_bounds__(256) void k_table_gfast(const double *__restrict__ lnK, double *__restrict__ lnKg, int Wpad, int G)
{
    __shared__ double tile[kMaxG][65];
    const int Gs = gfast_stride(G);
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;      // 64 x 4
    const size_t q = blockIdx.x;
    const int w0 = blockIdx.y * 64;
    for (int g = ty; g < G; g += 4) tile[g][tx] = lnK[(q * G + g) * Wpad + w0 + tx];
    __syncthreads();
    const double boxed0 = __longlong_as_double(0x7FF8000000000000LL);      // encode_lnk(0)
    double *dst = lnKg + (q * Wpad + w0) * Gs;
    for (int i = threadIdx.x; i < 64 * Gs; i += 256) {
        const int w = i / Gs, g = i - w * Gs;
        dst[i] = g < G ? tile[g][w] : boxed0;
    }
}

__global__ void k_table_check(const double *__restrict__ K, int W, int G, int Q, int *flag)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)W * Q) return;
    const int q = (int)(idx % Q);
    const size_t w = idx / Q;
    const double *src = K + w * (size_t)G * Q + q;
    bool bad = false, boxed = false;
    double prev = 0.0;
    for (int g = 0; g < G; ++g) {
        const double k = src[(size_t)g * Q];
        bad |= !(k >= 0.0) || (g > 0 && k < prev);
        boxed |= !(k > 0.0);
        prev = k;
    }
    if (bad) atomicOr(flag, 1);
    if (boxed) atomicOr(flag, 2);
}

// Array-level seam calc_k / calc_kg: writes the reference layout k[W][G][L][S] directly.
__global__ void k_calc_k_seam(const double *__restrict__ lnK, int W, int Wpad, int G, int NT, int S,
                              int L, const LayerInterp *__restrict__ li, double *__restrict__ k_out,
                              double *__restrict__ dk_out)
{
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t total = (size_t)L * S * G * W;
    if (idx >= total) return;
    int w = (int)(idx % W);
    size_t r = idx / W;
    int g = (int)(r % G); r /= G;
    int s = (int)(r % S);
    int l = (int)(r / S);
    LayerInterp q = li[l];
    size_t strideT = (size_t)S * G * Wpad;
    size_t off = ((size_t)s * G + g) * Wpad + w;
    double l1 = lnK[((size_t)q.ipl * NT + q.itl) * strideT + off];
    double l2 = lnK[((size_t)q.ipl * NT + q.ith) * strideT + off];
    double h1 = lnK[((size_t)q.iph * NT + q.itl) * strideT + off];
    double h2 = lnK[((size_t)q.iph * NT + q.ith) * strideT + off];
    double kk, dk;
    interp_kg(l1, l2, h1, h2, q.v, q.u, q.dudt, kk, dk);
    size_t o = (((size_t)w * G + g) * L + l) * S + s;
    k_out[o] = kk;
    if (dk_out) dk_out[o] = dk;
}

// internal dk[L][NP1][G][Wpad] -> reference dk[W][G][L][NP1]   (array-level k_overlapg seam)
__global__ void k_dk_to_ref(const double *__restrict__ src, double *__restrict__ dst, int W, int Wpad, int G,
                            int L, int NP1)
{
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t total = (size_t)W * G * L * NP1;
    if (idx >= total) return;
    int pp = (int)(idx % NP1);
    size_t r = idx / NP1;
    int l = (int)(r % L); r /= L;
    int g = (int)(r % G);
    int w = (int)(r / G);
    dst[idx] = src[(((size_t)l * NP1 + pp) * G + g) * Wpad + w];
}

// ------------------------------------------------------------------------------------------------
// .kta file block -> lnK.  The file stores k * 1e20 as float32 in the order [wave][press][temp][g] (Spectroscopy_0
// .read_ktable :2829-2850); the reader divides the float32 array by the Python float 1e20, which NumPy does in float32.
// One gas per launch: kf = the selected wavenumbers' block, as read.  Pad lanes (w >= W) get k = 0.  flag[0] |= 1: an entry
// < 0 / NaN or decreasing in g; |= 2: an entry that encode_lnk boxes (k <= 0 or NaN).
// ------------------------------------------------------------------------------------------------
__global__ void k_kta_relayout(const float *__restrict__ kf, double *__restrict__ lnK, int W, int Wpad, int G, int NP,
                               int NT, int S, int s, int *flag)
{
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t total = (size_t)NP * NT * G * Wpad;
    if (idx >= total) return;
    const int w = (int)(idx % Wpad);
    size_t r = idx / Wpad;
    const int g = (int)(r % G); r /= G;
    const int t = (int)(r % NT);
    const int p = (int)(r / NT);
    double k = 0.0;
    if (w < W) {
        const size_t src = (((size_t)w * NP + p) * NT + t) * G + g;
        const float q = kf[src] / 1.0e20f;
        k = (double)q;
        bool bad = !(k >= 0.0);
        if (g > 0 && q < kf[src - 1] / 1.0e20f) bad = true;
        if (bad) atomicOr(flag, 1);
        if (!(k > 0.0)) atomicOr(flag, 2);          // a boxed entry (pad lanes do not count)
    }
    lnK[((((size_t)p * NT + t) * S + s) * G + g) * Wpad + w] = encode_lnk(k);
}

// ------------------------------------------------------------------------------------------------
// Layer de-duplication inside a batch of atmospheric states.  The states of a numerical Jacobian differ from
// the unperturbed one at a single profile level, i.e. in two or three layers; every other layer has bit-identical
// (pressure, temperature, amounts) and therefore bit-identical gas opacities.  k_dedup_mark compares each layer
// (m, l) of models m >= 1 with layer l of model 0 and hands out rows of the opacity buffer: row l for a copy,
// a fresh row (atomic counter) otherwise.  k_dedup_gather packs the inputs of the rows that have to be computed
// so that the merge kernel sees them as the layers of one pseudo-model; k_thermal_rt follows tau_slot.
// Nothing is approximated: a layer is shared only when all of its S+2 inputs are equal to the last bit.
// ------------------------------------------------------------------------------------------------
// DedupCols: further per-layer inputs that are part of a row's identity, each an array [n][L][width] -- what the continuum of
// a row is formed from inside the call (ansfm_cirsrad_ck_thermal_ray_dev: the column and the Rayleigh composition;
// ansfm_cirsrad_ck_thermal_cont_dev: also the mixing ratios, para-H2 fraction and thickness behind the CIA term and the
// aerosol columns).  A state that perturbs He changes no spectroscopic amount, yet it changes CIA.
constexpr int kDedupCols = 8;
struct DedupCols {
    const double *p[kDedupCols];
    int width[kDedupCols];
    int n = 0;
    void add(const double *x, int w) { if (x && w > 0 && n < kDedupCols) { p[n] = x; width[n] = w; ++n; } }
};

__global__ void k_dedup_mark(int n_models, int L, int S, const double *__restrict__ press,
                             const double *__restrict__ temp, const double *__restrict__ amount,
                             int32_t *__restrict__ slot, int32_t *__restrict__ work, int *__restrict__ counter, DedupCols extra)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_models * L) return;
    const int m = i / L, l = i % L;
    if (m == 0) { slot[i] = l; work[l] = i; return; }
    auto bits = [](double x) { return __double_as_longlong(x); };
    bool same = bits(press[i]) == bits(press[l]) && bits(temp[i]) == bits(temp[l]);
#pragma unroll
    for (int k = 0; k < kDedupCols; ++k) {        // unrolled: the list stays in the kernel's arguments
        if (k >= extra.n || !same) break;
        const int wd = extra.width[k];
        const double *a = extra.p[k] + (size_t)i * wd, *b = extra.p[k] + (size_t)l * wd;
        for (int c = 0; c < wd && same; ++c) same = bits(a[c]) == bits(b[c]);
    }
    for (int s = 0; s < S && same; ++s)
        same = bits(amount[((size_t)m * S + s) * L + l]) == bits(amount[(size_t)s * L + l]);
    if (same) { slot[i] = l; return; }
    const int w = L + atomicAdd(counter, 1);
    slot[i] = w;
    work[w] = i;                                  // (m, l) flattened
}

__global__ void k_dedup_gather(int nwork, int L, int S, const int32_t *__restrict__ work, const double *__restrict__ press,
                               const double *__restrict__ temp, const double *__restrict__ amount,
                               double *__restrict__ press_w, double *__restrict__ temp_w, double *__restrict__ amount_w)
{
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nwork) return;
    const int i = work[w], m = i / L, l = i % L;
    press_w[w] = press[i];
    temp_w[w] = temp[i];
    for (int s = 0; s < S; ++s) amount_w[(size_t)s * nwork + w] = amount[((size_t)m * S + s) * L + l];
}

// [rows][G][Wpad] addressed through slot[L] -> reference TAUGAS[W][G][L]
__global__ void k_taugas_from_slots(const double *__restrict__ src, const int32_t *__restrict__ slot, double *__restrict__ dst,
                                    int W, int Wpad, int L, int G)
{
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)W * G * L) return;
    const int l = (int)(idx % L), g = (int)((idx / L) % G), w = (int)(idx / ((size_t)L * G));
    dst[idx] = src[((size_t)slot[l] * G + g) * Wpad + w];
}

// ------------------------------------------------------------------------------------------------
// K11: LBL-table mode (ILBL = LINE_BY_LINE_TABLES): Spectroscopy_0.calc_klbl :1768-1919 /
// calc_klblg :1601-1765 and the gas sum of calculate_gaseous_line_opacity (:3795-3817).
// The table is stored like the k-table with G = 1: lnK[NP][NTa][S][1][Wpad].
// ------------------------------------------------------------------------------------------------
struct LblInterp {
    int ip, a1, b1, a2, b2;   // corner temperature indices (a = it with python wrap, b = it+1)
    double v, u1, u2, omu1, omu2, du1, du2;
};

__device__ __forceinline__ int searchsorted_left_dev(const double *a, int n, double x)
{
    int lo = 0, hi = n;
    while (lo < hi) { int mid = (lo + hi) >> 1; if (a[mid] < x) lo = mid + 1; else hi = mid; }
    return lo;
}

// One thread per (model, layer).  TEMP is [NTa] or, when temp2d (the reference's NT < 0), [NP][NTa].
// with_grad selects calc_klblg's bracket (no it<0 clamp: python [-1] wrap, :1672-1675).
__global__ void k_layer_prep_lbl(int n_layers_total, const double *__restrict__ lay_press,
                                 const double *__restrict__ lay_temp, int NP, const double *__restrict__ PRESS,
                                 int NTa, const double *__restrict__ TEMP, int temp2d, double press_div,
                                 int grid_f32, int with_grad, LblInterp *__restrict__ out)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_layers_total) return;
    auto lg = [&](double x) { double r = log(x); return grid_f32 ? (double)(float)r : r; };
    double pmin = __builtin_inf(), pmax = -__builtin_inf();
    for (int k = 0; k < NP; ++k) { double l = lg(PRESS[k]); pmin = fmin(pmin, l); pmax = fmax(pmax, l); }
    double p_l = log(lay_press[i] / press_div);
    bool pcl = false, tcl = false;
    if (p_l < pmin) { p_l = pmin; pcl = true; }
    if (p_l > pmax) { p_l = pmax; pcl = true; }
    const int nt_all = temp2d ? NP * NTa : NTa;
    double tmin = __builtin_inf(), tmax = -__builtin_inf();
    for (int k = 0; k < nt_all; ++k) { tmin = fmin(tmin, TEMP[k]); tmax = fmax(tmax, TEMP[k]); }
    double t_l = lay_temp[i];
    if (t_l < tmin) { t_l = tmin; tcl = true; }
    if (t_l > tmax) { t_l = tmax; tcl = true; }
    // searchsorted(log PRESS, p_l) - 1 on the (ascending) log grid
    int lo = 0, hi = NP;
    while (lo < hi) { int mid = (lo + hi) >> 1; if (lg(PRESS[mid]) < p_l) lo = mid + 1; else hi = mid; }
    int ip = lo - 1;
    if (ip < 0) ip = 0;
    if (ip >= NP - 1) ip = NP - 2;
    const double l0 = lg(PRESS[ip]), l1 = lg(PRESS[ip + 1]);
    const double pden = grid_f32 ? (double)((float)l1 - (float)l0) : l1 - l0;
    LblInterp r;
    r.ip = ip;
    r.v = (grid_f32 && pcl) ? (double)(((float)p_l - (float)l0) / (float)pden) : (p_l - l0) / pden;
    for (int side = 0; side < 2; ++side) {
        const double *T = temp2d ? TEMP + (size_t)(ip + side) * NTa : TEMP;
        int it = searchsorted_left_dev(T, NTa, t_l) - 1;
        if (!with_grad && it < 0) it = 0;
        if (it >= NTa - 1) it = NTa - 2;
        const int itw = it < 0 ? it + NTa : it, itn = it + 1;
        const double den = grid_f32 ? (double)((float)T[itn] - (float)T[itw]) : T[itn] - T[itw];
        double u = (t_l - T[itw]) / den, omu;
        if (grid_f32 && tcl) {
            const float uf = ((float)t_l - (float)T[itw]) / (float)den;
            u = (double)uf;
            omu = (double)(1.0f - uf);
        } else
            omu = 1.0 - u;
        const double du = grid_f32 ? (double)(1.0f / (float)den) : 1. / den;
        if (side) { r.a2 = itw; r.b2 = itn; r.u2 = u; r.omu2 = omu; r.du2 = du; }
        else { r.a1 = itw; r.b1 = itn; r.u1 = u; r.omu1 = omu; r.du1 = du; }
    }
    out[i] = r;
}

__device__ __forceinline__ void interp_klbl(double l1, double l2, double h1, double h2, const LblInterp &q,
                                            double &kk, double &dk)
{   // l1 = (ip,it1) l2 = (ip,it1+1) h1 = (ip+1,it2) h2 = (ip+1,it2+1)      :1898-1917 / :1727-1762
    const bool b1 = lnk_is_boxed(l1), b2 = lnk_is_boxed(l2), b3 = lnk_is_boxed(h1), b4 = lnk_is_boxed(h2);
    kk = 0.0; dk = 0.0;
    const double omv = 1.0 - q.v;
    if (!(b1 | b2 | b3 | b4)) {
        kk = exp(omv * q.omu1 * l1 + q.v * q.omu2 * h1 + q.v * q.u2 * h2 + omv * q.u1 * l2);
        dk = kk * (-l1 * omv * q.du1 - h1 * q.v * q.du2 + h2 * q.v * q.du2 + l2 * omv * q.du1);
    } else if (b1 & b2 & b3 & b4) {
        const double klo1 = lnk_unbox(l1), klo2 = lnk_unbox(l2), khi1 = lnk_unbox(h1), khi2 = lnk_unbox(h2);
        kk = omv * q.omu1 * klo1 + q.v * q.omu2 * khi1 + q.v * q.u2 * khi2 + omv * q.u1 * klo2;
        dk = -klo1 * omv * q.du1 - khi1 * q.v * q.du2 + khi2 * q.v * q.du2 + klo2 * omv * q.du1;
    }
}

// array-level seam: k[W][L][S] (+dkdT)
__global__ void k_calc_klbl_seam(const double *__restrict__ lnK, int W, int Wpad, int NTa, int S, int L,
                                 const LblInterp *__restrict__ li, double *__restrict__ k_out,
                                 double *__restrict__ dk_out)
{
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t total = (size_t)L * S * W;
    if (idx >= total) return;
    const int w = (int)(idx % W);
    const int s = (int)((idx / W) % S);
    const int l = (int)(idx / ((size_t)W * S));
    const LblInterp q = li[l];
    const size_t strideT = (size_t)S * Wpad, off = (size_t)s * Wpad + w;
    const double l1 = lnK[((size_t)q.ip * NTa + q.a1) * strideT + off];
    const double l2 = lnK[((size_t)q.ip * NTa + q.b1) * strideT + off];
    const double h1 = lnK[((size_t)(q.ip + 1) * NTa + q.a2) * strideT + off];
    const double h2 = lnK[((size_t)(q.ip + 1) * NTa + q.b2) * strideT + off];
    double kk, dk;
    interp_klbl(l1, l2, h1, h2, q, kk, dk);
    const size_t o = ((size_t)w * L + l) * S + s;
    k_out[o] = kk;
    if (dk_out) dk_out[o] = dk;
}

// fused: tau[n][L][1][Wpad] = sum_s k_s * amount_s ; dk[n][L][S+1][1][Wpad]: slot s = k_s, slot S = sum dkdT_s*amount_s
__global__ void k_lbl_tau(const double *__restrict__ lnK, int Wpad, int NTa, int S, int L, int n_models,
                          const LblInterp *__restrict__ li, const double *__restrict__ amount,
                          double *__restrict__ tau, double *__restrict__ dk)
{
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t total = (size_t)n_models * L * Wpad;
    if (idx >= total) return;
    const int w = (int)(idx % Wpad);
    const int l = (int)((idx / Wpad) % L);
    const int m = (int)(idx / ((size_t)Wpad * L));
    const LblInterp q = li[(size_t)m * L + l];
    const size_t strideT = (size_t)S * Wpad;
    double t = 0.0, dT = 0.0;
    for (int s = 0; s < S; ++s) {
        const size_t off = (size_t)s * Wpad + w;
        const double l1 = lnK[((size_t)q.ip * NTa + q.a1) * strideT + off];
        const double l2 = lnK[((size_t)q.ip * NTa + q.b1) * strideT + off];
        const double h1 = lnK[((size_t)(q.ip + 1) * NTa + q.a2) * strideT + off];
        const double h2 = lnK[((size_t)(q.ip + 1) * NTa + q.b2) * strideT + off];
        double kk, dkk;
        interp_klbl(l1, l2, h1, h2, q, kk, dkk);
        const double am = amount[((size_t)m * S + s) * L + l];
        t += kk * am;                                   // TAUGAS[:,0,:,i] = k*VLOSDENS ; np.sum(TAUGAS,3)  :3810,:3817
        if (dk) {
            dk[(((size_t)m * L + l) * (S + 1) + s) * Wpad + w] = kk;     // :3813
            dT += dkk * am;                                              // :3814
        }
    }
    tau[((size_t)m * L + l) * Wpad + w] = t;
    if (dk) dk[(((size_t)m * L + l) * (S + 1) + S) * Wpad + w] = dT;
}

// ------------------------------------------------------------------------------------------------
// layout helpers (host-pointer seams): src[W][X1][X2] -> dst[(x1,x2 or x2,x1)][Wpad]
// ------------------------------------------------------------------------------------------------
// blockIdx.z = model of a batch (src_stride / dst_stride elements apart; 0 for a single array).
// Through a 32 x 32 LDS tile: block (32, 8); grid (Wpad / 32, ceil(X1 X2 / 32), batch).  Reads run along x (the source's
// fastest axis), writes along w.
__global__ __launch_bounds__(256) void k_transpose_w_last(const double *__restrict__ src, double *__restrict__ dst, int W, int Wpad,
                                                          int X1, int X2, int swap12, double padval, size_t src_stride,
                                                          size_t dst_stride)
{
    __shared__ double tile[32][33];
    const int X = X1 * X2;
    src += (size_t)blockIdx.z * src_stride;
    dst += (size_t)blockIdx.z * dst_stride;
    const int w0 = blockIdx.x * 32, x0 = blockIdx.y * 32;
    const int tx = threadIdx.x, ty = threadIdx.y;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int w = w0 + ty + 8 * k, x = x0 + tx;
        tile[ty + 8 * k][tx] = (w < W && x < X) ? src[(size_t)w * X + x] : padval;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = x0 + ty + 8 * k;           // source column = x1 * X2 + x2
        if (x < X) {
            const int row = swap12 ? (x % X2) * X1 + x / X2 : x;
            dst[(size_t)row * Wpad + w0 + tx] = tile[tx][ty + 8 * k];
        }
    }
}
// src[X1][X2][Wpad] -> dst[W][X1][X2]  (swap12: dst[W][X2][X1])
__global__ void k_w_to_first(const double *__restrict__ src, double *__restrict__ dst, int W, int Wpad,
                             int X1, int X2, int swap12)
{
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t total = (size_t)W * X1 * X2;
    if (idx >= total) return;
    int w = (int)(idx / ((size_t)X1 * X2));
    int r = (int)(idx % ((size_t)X1 * X2));
    int x1, x2;
    if (swap12) { x1 = r % X1; x2 = r / X1; }
    else { x2 = r % X2; x1 = r / X2; }
    dst[idx] = src[((size_t)x1 * X2 + x2) * Wpad + w];
}
// k[W][G][L][S] (reference layout) -> kin[S][L][G][Wpad]
__global__ void k_kin_permute(const double *__restrict__ src, double *__restrict__ dst, int W, int Wpad,
                              int G, int L, int S)
{
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t total = (size_t)S * L * G * Wpad;
    if (idx >= total) return;
    int w = (int)(idx % Wpad);
    size_t r = idx / Wpad;
    int g = (int)(r % G); r /= G;
    int l = (int)(r % L);
    int s = (int)(r / L);
    dst[idx] = (w < W) ? src[(((size_t)w * G + g) * L + l) * S + s] : 0.0;
}

}  // namespace ansfm

// ansfm_lblrt_kernels.hip.h -- the gas sum of the runtime line-by-line mode (ILBL = LINE_BY_LINE_RUNTIME) on gfx950.
//
// Restates the ILBL = 1 branch of ForwardModel_0.calculate_gaseous_line_opacity (ForwardModel_0.py:3819-3848) on the
// cross-sections that the line source left in HBM: krows[R][H][nw], one row per distinct (gas, p, T, mix fractions), H = 2
// when the (T + 5 K, p) spectrum of Spectroscopy_0.calc_klblg_online (:2019-2041) stands behind every row.
//
// Both kernels are wavenumber-fastest: a wave owns 64 consecutive wavenumbers of one (model, layer) -- Wpad is a multiple
// of 64, so the row index and the amount are the same in all its lanes (scalar loads) and every read of a k row and every
// write of tau / dk is one 512-byte run.  The k rows keep the accumulate kernels' pitch nw, so a read may start off a
// 128-byte line; it stays one run.
//
// The temperature derivative is the reference's, not a per-layer difference quotient: calc_klblg_online clears its T + 5 K
// buffer k1 once per gas, ahead of the loop over the points (Spectroscopy_0.py:1987 against :1992), so at point i it holds the
// T + 5 K spectra of the points 0 .. i, and dkdt[:, i] = (sum_{j <= i} k+_j - k_i) / 5 (:2041).  Both kernels form that sum, in
// ascending j as the reference's buffer grows.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ansfm {

// tau[n][L][1][Wpad] = sum_s k_s * amount_s in ascending s (:3841, :3848); dk[n][L][S + 1][1][Wpad]: slot s = k_s (:3844), slot
// S = sum_s dkdt_s * amount_s with dkdt_s of layer l = (sum_{j <= l} k+_s(layer j) - k_s(layer l)) / 5 (:2041, :3845) -- the
// layout k_lbl_tau writes.  The pad lanes w >= W hold 0.
__global__ __launch_bounds__(256) void k_lblrt_tau(const double *__restrict__ krows, int H, int W, int Wpad, int S, int L,
                                                   int n_models, const int32_t *__restrict__ krow,
                                                   const double *__restrict__ amount, double *__restrict__ tau,
                                                   double *__restrict__ dk)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)n_models * L * Wpad) return;
    const int w = (int)(idx % Wpad);
    const size_t ml = idx / Wpad;
    const int l = (int)(ml % L), m = (int)(ml / L);
    const bool in = w < W;
    double t = 0.0, dT = 0.0;
    for (int s = 0; s < S; ++s) {
        const size_t a = ((size_t)m * S + s) * L + l;
        const double *kr = krows + (size_t)krow[a] * H * W;
        const double am = amount[a];
        const double kk = in ? kr[w] : 0.0;
        t += kk * am;
        if (dk) {
            dk[(ml * (S + 1) + s) * Wpad + w] = kk;
            double k1 = 0.0;                                       // the reference's k1 at this layer
            if (in)
                for (int j = 0; j <= l; ++j) k1 += krows[((size_t)krow[a - l + j] * H + 1) * W + w];
            dT += ((k1 - kk) / 5.0) * am;
        }
    }
    tau[ml * Wpad + w] = t;
    if (dk) dk[(ml * (S + 1) + S) * Wpad + w] = dT;
}

// array-level seams: k[W][L][S] (+ dkdT, see above) from the rows (s, l) -> krows[s L + l]
__global__ void k_lblrt_seam(const double *__restrict__ krows, int H, int W, int S, int L, double *__restrict__ k_out,
                             double *__restrict__ dk_out)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)S * L * W) return;
    const int w = (int)(idx % W);
    const int l = (int)((idx / W) % L);
    const int s = (int)(idx / ((size_t)W * L));
    const double *kr = krows + ((size_t)s * L + l) * H * W;
    const double kk = kr[w];
    const size_t o = ((size_t)w * L + l) * S + s;
    k_out[o] = kk;
    if (dk_out) {
        double k1 = 0.0;
        for (int j = 0; j <= l; ++j) k1 += krows[(((size_t)s * L + j) * H + 1) * W + w];
        dk_out[o] = (k1 - kk) / 5.0;
    }
}

// side product of a gradient call: internal dk[L][NP1][G][Wpad] -> reference order [W][G][NP1][L]
__global__ void k_dtaugas_to_ref(const double *__restrict__ dk, double *__restrict__ out, int W, int Wpad, int G, int NP1, int L)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)W * G * NP1 * L) return;
    const int l = (int)(idx % L);
    const int s = (int)((idx / L) % NP1);
    const int g = (int)((idx / ((size_t)L * NP1)) % G);
    const int w = (int)(idx / ((size_t)L * NP1 * G));
    out[idx] = dk[(((size_t)l * NP1 + s) * G + g) * Wpad + w];
}

}  // namespace ansfm

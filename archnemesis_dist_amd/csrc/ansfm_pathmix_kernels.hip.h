// ansfm_pathmix_kernels.hip.h -- the device code the fused gradient routes share (transit, occultation, limb, disc; kernels in
// ansfm_transit_kernels.hip.h, ansfm_occultation_kernels.hip.h, ansfm_limb_kernels.hip.h, ansfm_disc_kernels.hip.h): the path
// pass exp(-tau_path), the
// contraction of the columns of a (layer, geometry) against the opacity derivatives of the gradient merge, and the sums over
// g that give the per-path spectra and MOD.  Device functions only, inlined into the kernels that call them; no kernel here.
// The functions read their arguments from the calling kernel's own params struct (OccParams, LimbParams, TransitParams, DiscParams) by
// field name; each says which fields.  Sums run in a fixed order and nothing is accumulated atomically: equal inputs, equal bits.
//
// LDS budget of the contraction (design statements, not measurements).  A block of 4 waves serves one (64-wavenumber tile,
// layer).  Its LDS holds a chunk of SC slots of the layer's slab of dk, SC x G x 512 B, read from HBM once per block and shared
// by every geometry, and one column set [G][64] per wave, 4 x G x 512 B.  The block is held to 80 KiB, half of the 160 KiB of a
// CU, so that two blocks (8 waves, 2 per SIMD) are resident and one block's staging of a chunk overlaps the other's contraction.
// At G = 20, S = 8: the waves' columns take 40 KiB, which leaves 40 KiB = 4 slots; the 9 slots go in 3 even chunks of 3
// (30 KiB + 40 KiB = 70 KiB a block, 2 blocks per CU).  Holding the whole slab (90 KiB + 40 KiB) would leave one block, 1 wave
// per SIMD, with nothing to hide the staging behind; a smaller budget (3 blocks at 53 KiB) would leave 1 slot a chunk and 9
// barrier pairs.  The price of a chunk is that a wave fills the columns of a geometry again.  Where G is so large that 80 KiB
// hold no slot beside the columns, the block takes up to 160 KiB.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "ansfm_merge_common.hip.h"
#include "ansfm_grad_slots.hip.h"

namespace ansfm {

constexpr int kMixWaves = 4;                       // waves of a contraction block (k_occ_grad, k_limb_grad, k_disc_grad)
constexpr size_t kMixLdsTwoBlocks = 80 * 1024;     // LDS of a block when two are to share a CU
constexpr size_t kMixLdsOneBlock = 160 * 1024;

// Slots of dk a chunk of the contraction stages and the LDS of its block: the largest chunk that fits the two-block budget
// beside the waves' columns (the one-block budget where that holds no slot), then evened out over the chunks it takes; 0: no fit.
inline int slab_chunk(int G, int NP1, size_t *lds_bytes)
{
    const size_t row = (size_t)G * kWave * sizeof(double), cols = kMixWaves * row;
    for (size_t budget : {kMixLdsTwoBlocks, kMixLdsOneBlock}) {
        if (budget < cols + row) continue;
        const int most = (int)std::min<size_t>((budget - cols) / row, (size_t)NP1);
        const int chunks = (NP1 + most - 1) / most, sc = (NP1 + chunks - 1) / chunks;
        *lds_bytes = cols + (size_t)sc * row;
        return sc;
    }
    return 0;
}

// The path pass of one wave per (wavenumber tile of 64, g), grid (Wpad / 64, G), block 64.  The LDS tile [L][64] holds the total
// opacity of every layer while the paths are summed through Sm compressed by path (col_ptr / col_lay / col_val); indices and
// values are uniform over the wave: the compiler fetches the indices with scalar loads and the values with vector loads from a
// scalar base.  tpart [P][G][Wpad] = exp(-tau_path).  A lane touches its own column of the tile and its own elements of tpart
// only, so no barrier is needed.  Reads q.tau, cont, col_ptr, col_lay, col_val, L, P, G, Wpad; writes q.tpart.
template <class Params> __device__ __forceinline__ void path_pass(const Params &q, double *tile)
{
    const int lane = threadIdx.x, g = blockIdx.y;
    const size_t nu = (size_t)blockIdx.x * kWave + lane;      // < Wpad: every array read or written here is padded to it
    const size_t GWp = (size_t)q.G * q.Wpad, at = (size_t)g * q.Wpad + nu;
    for (int l = 0; l < q.L; ++l)
        tile[l * kWave + lane] = q.tau[(size_t)l * GWp + at] + (q.cont ? q.cont[(size_t)l * q.Wpad + nu] : 0.0);
    for (int p = 0; p < q.P; ++p) {
        const int i1 = q.col_ptr[p + 1];
        double t = 0.0;
#pragma unroll 4
        for (int i = q.col_ptr[p]; i < i1; ++i) t += q.col_val[i] * tile[q.col_lay[i] * kWave + lane];
        q.tpart[(size_t)p * GWp + at] = exp(-t);
    }
}

// xfac of a lane's wavenumber; 0 on the padding lanes, whose results are not stored
__device__ __forceinline__ double mix_factor(const double *xfac, size_t nu, int W)
{
    return nu < (size_t)W ? (xfac ? xfac[nu] : 1.0) : 0.0;
}

// The contraction of one block of kMixWaves waves per (wavenumber tile, layer l = blockIdx.y); lanes run over wavenumbers.  The
// slots of the layer's slab of dk are staged in LDS in chunks of q.SC (slots the gas selection leaves out are neither staged nor
// read).  The geometries with has_entry(l, iq) are dealt to the waves in turn; for each of its geometries a wave has
// fill_columns(iq, wg, Xs) put the g-weighted columns [G][64] into its own LDS columns wg (element wg[g * 64 + lane]) and their
// sum over g, for the continuum terms, into Xs; it contracts every parameter whose slot lies in the chunk against the staged
// slab, goes through dtau_param_gsum, has finish(v, kpar, iq) complete the value, sets NaN to 0 (nan_to_num, :4507) and writes
// dMOD[w][k][l][q].  Parameters without a slot are written with the first chunk.  A geometry without an entry in the layer
// gets zeros and no call of fill_columns.  grid (Wpad / 64, L), block 256, LDS (SC + kMixWaves) x G x 512 B.
// Reads q.dk, dcont, dcont_gas, slot_of_param, gas_mask, SC, W, Wpad, G, L, Q, NPAR, NVMR, NP1; writes q.dmod.
template <class Params, class HasEntry, class FillColumns, class Finish>
__device__ __forceinline__ void mix_contract(const Params &q, double *lds, HasEntry has_entry, FillColumns fill_columns, Finish finish)
{
    const int lane = threadIdx.x & (kWave - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave), l = blockIdx.y;
    const int G = q.G, NP1 = q.NP1, Q = q.Q;
    const size_t nu = (size_t)blockIdx.x * kWave + lane;
    const size_t GWp = (size_t)G * q.Wpad;
    const bool live = nu < (size_t)q.W;
    double *slab = lds, *wg = lds + (size_t)q.SC * G * kWave + (size_t)wave * G * kWave;
    const double *dkl = q.dk + (size_t)l * NP1 * GWp + (size_t)blockIdx.x * kWave;

    for (int c0 = 0; c0 < NP1; c0 += q.SC) {
        const int cn = min(q.SC, NP1 - c0);
        if (c0) __syncthreads();                                   // every wave is done with the chunk before
        for (int row = wave; row < cn * G; row += kMixWaves) {      // row = (slot - c0) G + g: 512 B of dk each
            const int s = c0 + row / G;
            if ((q.gas_mask >> (s == NP1 - 1 ? 31 : s)) & 1u)
                slab[row * kWave + lane] = dkl[((size_t)c0 * G + row) * q.Wpad + lane];
        }
        __syncthreads();
        int n = 0;
        for (int iq = 0; iq < Q; ++iq) {
            if (!has_entry(l, iq)) {                               // no path of this geometry crosses the layer
                if (c0 == 0 && iq % kMixWaves == wave && live)
                    for (int kpar = 0; kpar < q.NPAR; ++kpar) q.dmod[((nu * q.NPAR + kpar) * q.L + l) * Q + iq] = 0.0;
                continue;
            }
            if (n++ % kMixWaves != wave) continue;
            double Xs = 0.0;
            fill_columns(iq, wg, Xs);
            for (int kpar = 0; kpar < q.NPAR; ++kpar) {
                const int slot = q.slot_of_param[kpar];
                if (slot < 0 ? c0 != 0 : (slot < c0 || slot >= c0 + cn)) continue;
                double ys = 0.0;
                if (slot >= 0) {
                    const double *sl = slab + (size_t)(slot - c0) * G * kWave + lane;
                    for (int g = 0; g < G; ++g) ys += wg[g * kWave + lane] * sl[g * kWave];
                }
                double v = finish(dtau_param_gsum(slot, ys, Xs, NP1, q.dcont, q.dcont_gas, (size_t)0, q.NPAR, q.NVMR, kpar, q.L, l,
                                                  q.Wpad, (int)nu),
                                  kpar, iq);
                if (v != v) v = 0.0;
                if (live) q.dmod[((nu * q.NPAR + kpar) * q.L + l) * Q + iq] = v;
            }
        }
    }
}

// What block row 0 of the contraction's grid adds, paths and geometries dealt to its waves: the per-path sums
// out_paths[w][p] = sum_g dg src[p][g][w] of src [P][G][Wpad], and their mix MOD[w][q] = xf sum_i C[q][p_i] (sum_g dg src[p_i]).
// Reads q.delg, mix_ptr, mix_path, mix_val, W, Wpad, G, P, Q; writes out_paths and q.mod.
template <class Params> __device__ __forceinline__ void mix_path_sums(const Params &q, const double *src, double xf, double *out_paths)
{
    const int lane = threadIdx.x & (kWave - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const int G = q.G, Q = q.Q;
    const size_t nu = (size_t)blockIdx.x * kWave + lane;
    const size_t GWp = (size_t)G * q.Wpad;
    const bool live = nu < (size_t)q.W;
    for (int p = wave; p < q.P; p += kMixWaves) {
        double s = 0.0;
        for (int g = 0; g < G; ++g) s += q.delg[g] * src[(size_t)p * GWp + (size_t)g * q.Wpad + nu];
        if (live) out_paths[nu * q.P + p] = s;
    }
    for (int iq = wave; iq < Q; iq += kMixWaves) {
        double m = 0.0;
        for (int i = q.mix_ptr[iq]; i < q.mix_ptr[iq + 1]; ++i) {
            double s = 0.0;
            for (int g = 0; g < G; ++g) s += q.delg[g] * src[(size_t)q.mix_path[i] * GWp + (size_t)g * q.Wpad + nu];
            m += q.mix_val[i] * s;
        }
        if (live) q.mod[nu * Q + iq] = xf * m;
    }
}

}  // namespace ansfm

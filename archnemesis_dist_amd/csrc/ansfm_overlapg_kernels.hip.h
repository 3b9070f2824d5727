// ansfm_overlapg_kernels.hip.h -- k_ck_overlapg, the gradient merge kernel, with its replay / resolve helpers
// (unit: ansfm_overlapg.hip).
#pragma once
#include "ansfm_merge64.hip.h"

namespace ansfm {

// ------------------------------------------------------------------------------------------------
// K1g+K2g fused: calc_kg + k_overlapg/rankg (ForwardModel_0.py:5842-6026).   "ck_overlapg"
//
// rankg accumulates, per output bin, weight * gradient-row of every element in sorted order
// (:6002-6025).  The gradient row of element (i, j) is (:5918-5921, :5946-5949)
//      slot pp <= igas : D_old[pp][i]          (previous stage's dk_g_param, by ROW)
//      slot igas+1     : k_new[j]              (by COLUMN)
//      slot igas+2     : D_old[igas+1][i] + dkdT_new[j]*amount
// so every slot is a weighted gather of a G-vector along the sorted order.  The merge runs ONCE (the
// forward kernel's loop) and records the order as 16 bits per step; the slots are then produced by
// replaying that order with up to three G-vectors staged in the LDS the merge no longer needs
// (gathers out of LDS [index][lane] are conflict-free; out of global memory they touch ~40 cache
// lines per wave-load).  Bin boundaries are deferred exactly like the forward walk: the replay stores the
// raw partial sums, a uniform 20-iteration pass applies frac / (1-frac) carry / normalisation.
// Slot bookkeeping of the skip branches (:5897-5937) is reproduced, including the stale slots they
// leave behind.
// ------------------------------------------------------------------------------------------------
struct OverlapGParams {
    OverlapParams o;          // o.scratch: [grid][G+1][6][64] bin records
    const double *dkin;       // FROM_K: dkdT[S][L][G][Wpad]
    double *dk;               // out [n][L][S+1][G][Wpad]
    double *gscratch;         // [grid][2 + 2*(S+1) + 1][G][64]   KRB, DTB, Dbuf0, Dbuf1, Asave
    unsigned long long *perm; // [grid][ceil(G*G/4)][64]: four 16-bit step codes per word
    unsigned gas_mask;        // bit s: the slot of gas s (d tau / d amount_s) is wanted.  A state vector names one or two gases:
                              // every other gas's slot would cost a replay pass per later merge for nothing (its rows of dk are
                              // written as zeros).  Bit 31: the temperature slot (two passes per merge).
};

// from_k (array-level k_overlapg seam) is a run-time flag here: the load phase is a few per cent of the kernel and one
// template parameter less halves the number of instantiations of the largest kernel of the library.
__device__ __forceinline__ void load_gas_g(const OverlapGParams &pg, const LayerInterp &q, int m, int l, int s,
                                           int nu, double *DST, double *KR, double *DT, int lane, bool &unsorted)
{
    const bool FROM_K = pg.o.kin != nullptr;
    const OverlapParams &p = pg.o;
    const int G = p.G;
    const double amt = p.amount[((size_t)m * p.S + s) * p.L + l];
    double prev = -__builtin_inf();
    if (FROM_K) {
        const size_t base = (((size_t)s * p.L + l) * G) * p.Wpad + nu;
        for (int g0 = 0; g0 < G; g0 += kLoadBatch) {
            double r1[kLoadBatch], r2[kLoadBatch];
#pragma unroll
            for (int k = 0; k < kLoadBatch; ++k) {
                const int gi = (g0 + k < G) ? g0 + k : G - 1;
                r1[k] = p.kin[base + (size_t)gi * p.Wpad];
                r2[k] = pg.dkin[base + (size_t)gi * p.Wpad];
            }
#pragma unroll
            for (int k = 0; k < kLoadBatch; ++k)
                if (g0 + k < G) {
                    const int g = g0 + k;
                    const double kk = r1[k] * amt;
                    DST[g * kWave + lane] = kk;
                    KR[g * kWave + lane] = r1[k];
                    DT[g * kWave + lane] = r2[k] * amt;
                    unsorted |= (kk < prev);
                    prev = kk;
                }
        }
    } else {
        const size_t strideT = (size_t)p.S * G * p.Wpad;
        const size_t off = (size_t)s * G * p.Wpad + nu;
        const double *c1 = p.lnK + ((size_t)q.ipl * p.NT + q.itl) * strideT + off;
        const double *c2 = p.lnK + ((size_t)q.ipl * p.NT + q.ith) * strideT + off;
        const double *c3 = p.lnK + ((size_t)q.iph * p.NT + q.itl) * strideT + off;
        const double *c4 = p.lnK + ((size_t)q.iph * p.NT + q.ith) * strideT + off;
        for (int g0 = 0; g0 < G; g0 += kLoadBatch) {
            double r1[kLoadBatch], r2[kLoadBatch], r3[kLoadBatch], r4[kLoadBatch];
#pragma unroll
            for (int k = 0; k < kLoadBatch; ++k) {
                const int gi = (g0 + k < G) ? g0 + k : G - 1;
                const size_t go = (size_t)gi * p.Wpad;
                r1[k] = __builtin_nontemporal_load(c1 + go);
                r2[k] = __builtin_nontemporal_load(c2 + go);
                r3[k] = __builtin_nontemporal_load(c3 + go);
                r4[k] = __builtin_nontemporal_load(c4 + go);
            }
#pragma unroll
            for (int k = 0; k < kLoadBatch; ++k)
                if (g0 + k < G) {
                    const int g = g0 + k;
                    double kraw, dkr;
                    interp_kg(r1[k], r2[k], r3[k], r4[k], q.v, q.u, q.dudt, kraw, dkr);
                    const double kk = kraw * amt;
                    DST[g * kWave + lane] = kk;
                    KR[g * kWave + lane] = kraw;
                    DT[g * kWave + lane] = dkr * amt;
                    unsorted |= (kk < prev);
                    prev = kk;
                }
        }
    }
}

// global [G][64] -> LDS [G][64], loads batched: one memory round trip per kStageBatch rows (every replay pass starts
// with one of these and the wave has at most one sibling to hide it behind)
constexpr int kStageBatch = 20;
__device__ __forceinline__ void stage_slice(double *dst_lds, const double *__restrict__ src, int G, int lane)
{
    for (int g0 = 0; g0 < G; g0 += kStageBatch) {
        double r[kStageBatch];
#pragma unroll
        for (int k = 0; k < kStageBatch; ++k)
            r[k] = gld<double>(src, (unsigned)(((g0 + k < G) ? g0 + k : G - 1) * kWave + lane) * 8u);
#pragma unroll
        for (int k = 0; k < kStageBatch; ++k)
            if (g0 + k < G) dst_lds[(g0 + k) * kWave + lane] = r[k];
    }
}

// generic path: LDS position g holds the value of the ORIGINAL g-ordinate P[g] (the column was sorted per lane)
__device__ __forceinline__ void stage_slice_perm(double *dst_lds, const double *__restrict__ src, const unsigned char *P,
                                                 int G, int lane)
{
    for (int g = 0; g < G; ++g) dst_lds[g * kWave + lane] = src[(size_t)P[g * kWave + lane] * kWave + lane];
}

constexpr int kCodesPerWord = 5;       // 12-bit step codes in a 64-bit word of the replay stream (60 bits used)
// Replay of the recorded order for one gathered vector: SL[row] (slots of the earlier gases, row part of the
// temperature slot) or, COL, SL[col] (the new gas's slot, column part of the temperature slot).
// Store-free and branch-free: the running sum is written every step to the LDS row of
// the lane's current bin, so each row ends up holding the sum before the element that closed the bin; global
// stores inside this loop would sit in front of the code-word loads in the (in-order) vmcnt queue.
// OUTL has G+1 rows (row G collects what follows the last bin).  Returns the sum after the last boundary.
template <bool COL, bool W32, bool SORTED = true>
__device__ __forceinline__ double grad_replay(int nloop, int lane, const unsigned long long *__restrict__ perm,
                                              const double *SL, double *OUTL, const double *DG,
                                              const unsigned char *PA = nullptr, const unsigned char *PB = nullptr)
{
    double acc = 0.0;
    unsigned bo = lds_addr(OUTL + lane);            // LDS byte address of the lane's slot in the row of its current bin
    const unsigned lane8 = (unsigned)lane * 8u;     // SL is the A region (offset kLdsA)
    // the steps of one code word: all LDS operands first (one LDS round trip per word), then the dependent part.
    // Field k of the word = bits [12k, 12k + 12): row, column, closed-a-bin.  The row / column are taken out already
    // multiplied by 4 (byte offsets into the float32 weight table; << 7 more = the row of an [index][lane] array).
    auto group = [&](unsigned long long word, int nst) {
        double g[kCodesPerWord], wr[kCodesPerWord];
        const unsigned wlo = (unsigned)word, whi = (unsigned)(word >> 32);
        const unsigned wmid = __builtin_amdgcn_alignbit(whi, wlo, 24);      // bits 24..55: the field across the two halves
        unsigned crs[kCodesPerWord];
#pragma unroll
        for (int k = 0; k < kCodesPerWord; ++k) {
            const unsigned src = (k < 2) ? wlo : (k == 2 ? wmid : whi);
            constexpr int offs[kCodesPerWord] = {0, 12, 0, 4, 16};
            const int off = offs[k];
            crs[k] = src & (0x400u << off);
            const unsigned r4 = (off >= 2 ? (src >> (off - 2)) : (src << (2 - off))) & 0x7Cu;
            const unsigned c4 = (src >> (off + 3)) & 0x7Cu;
            if constexpr (SORTED) {
                if constexpr (W32) wr[k] = (double)(lds_ldf(kLdsDGF + r4) * lds_ldf(kLdsDGF + c4));
                else wr[k] = lds_ld(kLdsDG + 2 * r4) * lds_ld(kLdsDG + 2 * c4);
            } else
                wr[k] = pair_weight<W32>(DG, PA[(r4 >> 2) * kWave + lane], PB[(c4 >> 2) * kWave + lane]);
            g[k] = lds_ld(kLdsA + (((COL ? c4 : r4) << 7) + lane8));
        }
#pragma unroll
        for (int k = 0; k < kCodesPerWord; ++k) {
            if (k < nst) {
                const bool cross = crs[k] != 0;
                lds_st(bo, acc);
                const double an = acc + g[k] * wr[k];
                acc = cross ? 0.0 : an;
                bo += cross ? kWave * 8u : 0u;
            }
        }
    };
    const int nfull = nloop / kCodesPerWord, ngrp = (nloop + kCodesPerWord - 1) / kCodesPerWord;
    // Code words are fetched kPF words (4*kPF steps) ahead into kPF statically named registers: no register
    // rotation (a move of the newest word would wait for its load) and no predicated loads (clamped index).
    constexpr int kPF = 4;
    unsigned long long q[kPF];
    const unsigned lane8p = (unsigned)lane * 8u;
#pragma unroll
    for (int k = 0; k < kPF; ++k) q[k] = gld<unsigned long long>(perm, (unsigned)(k < ngrp ? k : ngrp - 1) * (kWave * 8u) + lane8p);
    int gidx = 0;
    for (; gidx + kPF <= nfull; gidx += kPF) {
#pragma unroll
        for (int j = 0; j < kPF; ++j) {
            const unsigned long long word = q[j];
            const int nxt = gidx + j + kPF;
            q[j] = gld<unsigned long long>(perm, (unsigned)(nxt < ngrp ? nxt : ngrp - 1) * (kWave * 8u) + lane8p);
            group(word, kCodesPerWord);
        }
    }
    // remaining full words and the partial last one (their loads are already in flight / clamped duplicates)
#pragma unroll
    for (int j = 0; j < kPF; ++j) {
        if (gidx + j < ngrp) {
            const int left = nloop - kCodesPerWord * (gidx + j);
            group(q[j], left < kCodesPerWord ? left : kCodesPerWord);
        }
    }
    return acc;
}

// deferred bin boundaries of one replayed vector.  The record of bin b is ONE 16-byte pair per lane, (frac, 1 / weight-sum), with
// the closing element's (row, column) in the 11 lowest mantissa bits of frac; its weight is re-formed from the tables.  (Four
// values in two pairs until the end of round 2: the records are read by every replay pass -- 49 per cell -- and with the step
// codes and the slot vectors they cycle through L2 at 5 TB/s, profiles/r02_grad_traffic.json: the kernel is bound by that
// stream.)  ACCUM: the column part of the temperature slot is added to the row part already in OUT.
template <bool COL, bool ACCUM, bool W32, bool SORTED>
__device__ __forceinline__ void grad_resolve(int G, int lane, int ig, const double *__restrict__ rec,
                                             const double *SL, const double *OUTL, double tail,
                                             double *__restrict__ OUT, const double *DG, const unsigned char *PA,
                                             const unsigned char *PB)
{
    double carry = 0.0;
    constexpr int kRB = 10;     // two memory round trips per pass for G = 20
    for (int b0 = 0; b0 < G; b0 += kRB) {
        double rfr[kRB], rri[kRB], rold[kRB];
#pragma unroll
        for (int k = 0; k < kRB; ++k) {
            const int bi = (b0 + k < G) ? b0 + k : G - 1;
            const dbl2 v0 = gld<dbl2>(rec, (unsigned)bi * kRecBin + (unsigned)lane * 16u);
            rfr[k] = v0.x; rri[k] = v0.y;
            if constexpr (ACCUM) rold[k] = gld<double>(OUT, (unsigned)(bi * kWave + lane) * 8u);
        }
#pragma unroll
        for (int k = 0; k < kRB; ++k) {
            const int b = b0 + k;
            if (b < G) {
                double v = 0.0;
                if (b < ig) {
                    const long long fb = __double_as_longlong(rfr[k]);
                    const unsigned code = (unsigned)fb & 0x7FFu;
                    const int crow = code & 31, ccol = (code >> 5) & 63;
                    rfr[k] = __longlong_as_double(fb & ~0x7FFLL);
                    double wk;
                    if constexpr (SORTED) wk = pair_weight<W32>(DG, crow, ccol);
                    else wk = pair_weight<W32>(DG, PA[crow * kWave + lane], PB[ccol * kWave + lane]);
                    const double g = SL[(COL ? ccol : crow) * kWave + lane];
                    const double gw = g * wk;
                    v = ((carry + OUTL[b * kWave + lane]) + rfr[k] * gw) * rri[k];
                    carry = (1.0 - rfr[k]) * gw;
                } else if (b == ig)
                    v = (carry + tail) * rri[k];
                if constexpr (ACCUM) v += rold[k];
                gst<double>(OUT, (unsigned)(b * kWave + lane) * 8u, v);
            }
        }
    }
}

// SORTED = false: generic path (k not non-decreasing in g), as in k_ck_overlap: A and B are sorted per lane, PA / PB give
// the original g-ordinate of each sorted position.  The gradient rows in the global scratch stay in ORIGINAL order while
// a spectrum is unmerged (rows and columns are staged through PA / PB for the replay) and are in bin order -- the
// identity -- after a merge.
template <int NR, bool W32, bool SORTED = true>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_ck_overlapg(OverlapGParams pg)
{
    const OverlapParams &p = pg.o;
    extern __shared__ double smem[];
    const int lane = threadIdx.x;
    const int G = p.G;
    const int NP1 = p.S + 1;
    // tables first: their LDS addresses are compile-time constants (dynamic LDS starts at 0), so a table read is
    // `ds_read vaddr = index << k, offset:const` with no base add
    double *DG = smem;                           // [kMaxG] doubles, then GORD [kMaxG + 2], then the float32 copy of DG
    double *GORD = DG + kMaxG;
    double *A = reinterpret_cast<double *>(reinterpret_cast<char *>(GORD + kMaxG + 2) + kMaxG * sizeof(float));
    double *B = A + G * kWave;                   // G+1 rows
    unsigned char *PA = reinterpret_cast<unsigned char *>(B + (G + 1) * kWave);   // SORTED = false only
    unsigned char *PB = PA + G * kWave;
    if (lds_addr(smem) != 0) {                   // the replay addresses the tables and A by literal LDS offsets
        if (lane == 0) atomicOr(p.err_flag, 2);
        return;
    }
    if (lane < G) {
        DG[lane] = p.del_g[lane];
        const_cast<float *>(delg_f32_table(DG))[lane] = (float)p.del_g[lane];
    }
    if (lane < G + 2) GORD[lane] = p.g_ord[lane];
    const double HUGE_KEY = __longlong_as_double(0x7FE0000000000000LL);
    __syncthreads();
    double wsum = 0.0;
    for (int g = 0; g < G; ++g) wsum += DG[g];
    const double wtot = wsum * wsum;

    double *rec = p.scratch + (size_t)blockIdx.x * 6 * (G + 1) * kWave;
    const size_t GW = (size_t)G * kWave;
    double *gs = pg.gscratch + (size_t)blockIdx.x * (3 + 2 * (size_t)NP1) * GW;
    double *KRB = gs, *DTB = gs + GW;
    // the two gradient-row buffers as offsets onto `gs`: indexing an array of pointers would lose the global address
    // space (flat loads / stores, which also tie up the LDS counter)
    const size_t dboff[2] = {2 * GW, (2 + (size_t)NP1) * GW};
    double *const Dbuf0 = gs + dboff[0];
    double *ASAVE = gs + (2 + 2 * (size_t)NP1) * GW;
    const int nloop = G * G;
    unsigned long long *perm = pg.perm + (size_t)blockIdx.x * ((nloop + kCodesPerWord - 1) / kCodesPerWord) * kWave;

    TileQueue tq;
    tq.init();
    for (;;) {
        int vt = 0, m = 0, l = 0;
        if (!tq.next(p, lane, vt, m, l)) break;
        const int nu = vt * kWave + lane;
        LayerInterp q;
        if (p.kin == nullptr) q = p.li[(size_t)m * p.L + l];
        bool unsorted = false;
        int cur = 0;
        // gas 0: a = k0*amount0 ; D[0] = k0 (d/d amount0), D[1] = dkdT0*amount0 (d/dT), rest 0
        load_gas_g(pg, q, m, l, 0, nu, A, Dbuf0, Dbuf0 + GW, lane, unsorted);
        double alast = A[(G - 1) * kWave + lane];       // last g-ordinate in the ORIGINAL order
        if constexpr (!SORTED) sort_column(A, PA, G, lane);
        for (int pp = 2; pp < NP1; ++pp)
            for (int g = 0; g < G; ++g) Dbuf0[(size_t)pp * GW + g * kWave + lane] = 0.0;

        for (int s = 1; s < p.S; ++s) {
            const int igas = s - 1;
            const int n = igas + 3;  // rankg's `n`
            load_gas_g(pg, q, m, l, s, nu, B, KRB, DTB, lane, unsorted);
            if constexpr (SORTED)                       // the call is rerun on the generic path: no point in merging
                if (__builtin_amdgcn_ballot_w64(unsorted) != 0) break;
            double *Dold = gs + (cur ? dboff[1] : dboff[0]), *Dnew = gs + (cur ? dboff[0] : dboff[1]);
            const double blast = B[(G - 1) * kWave + lane];
            if constexpr (!SORTED) sort_column(B, PB, G, lane);
            if constexpr (SORTED) alast = A[(G - 1) * kWave + lane];
            bool takeB, keepA;
            if (s == 1) { takeB = (alast <= 0.0); keepA = !takeB && (blast <= 0.0); }
            else { keepA = (blast <= 0.0); takeB = !keepA && (alast <= 0.0); }
            const bool do_merge = !(takeB | keepA);
            if (!do_merge) {
                // skip branches :5897-5907, :5930-5937 (slots beyond the ones written keep their old content)
                for (int pp = 0; pp < NP1; ++pp)
                    for (int g = 0; g < G; ++g) {
                        const size_t o = (size_t)pp * GW + g * kWave + lane;
                        double v = Dold[o];
                        if (keepA) {
                            if (pp == igas + 2) v = Dold[(size_t)(igas + 1) * GW + g * kWave + lane];
                            else if (pp == igas + 1) v = 0.0;
                        } else {  // takeB
                            if (pp == igas + 1) v = KRB[g * kWave + lane];
                            else if (pp == igas + 2) v = DTB[g * kWave + lane];
                            else if (s == 1 && pp == 0) v = 0.0;
                        }
                        Dnew[o] = v;
                    }
                if (takeB) {
                    for (int g = 0; g < G; ++g) A[g * kWave + lane] = B[g * kWave + lane];
                    if constexpr (!SORTED) {
                        for (int g = 0; g < G; ++g) PA[g * kWave + lane] = PB[g * kWave + lane];
                        alast = blast;
                    }
                }
            } else {
                // ---- the forward merge, recording the order -------------------------------------------------
                B[G * kWave + lane] = HUGE_KEY;
                double R[NR];
                merge_init<NR>(R, G, lane, A, B[lane], HUGE_KEY);
                MergeElem e0, e1;
                merge_fetch<W32, SORTED>(R[0], lane, A, B, DG, e0, PA, PB);
                WalkState ws = walk_begin(GORD, lane);
                unsigned long long *pw = perm + lane;
                int it = 0;
                auto put5 = [&](unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned c4) {
                    *reinterpret_cast<uint2 *>(pw) = make_uint2(c0 | (c1 << 12) | (c2 << 24), (c2 >> 8) | (c3 << 4) | (c4 << 16));
                    pw += kWave;
                };
                // five 12-bit codes per word; the two element registers swap roles every step, so ten steps are written out
                for (; it + 9 < nloop; it += 10) {
                    const unsigned c0 = merge_step<NR, W32, true, SORTED>(R, e0, e1, ws, lane, A, B, DG, GORD, rec, PA, PB);
                    const unsigned c1 = merge_step<NR, W32, true, SORTED>(R, e1, e0, ws, lane, A, B, DG, GORD, rec, PA, PB);
                    const unsigned c2 = merge_step<NR, W32, true, SORTED>(R, e0, e1, ws, lane, A, B, DG, GORD, rec, PA, PB);
                    const unsigned c3 = merge_step<NR, W32, true, SORTED>(R, e1, e0, ws, lane, A, B, DG, GORD, rec, PA, PB);
                    const unsigned c4 = merge_step<NR, W32, true, SORTED>(R, e0, e1, ws, lane, A, B, DG, GORD, rec, PA, PB);
                    put5(c0, c1, c2, c3, c4);
                    const unsigned c5 = merge_step<NR, W32, true, SORTED>(R, e1, e0, ws, lane, A, B, DG, GORD, rec, PA, PB);
                    const unsigned c6 = merge_step<NR, W32, true, SORTED>(R, e0, e1, ws, lane, A, B, DG, GORD, rec, PA, PB);
                    const unsigned c7 = merge_step<NR, W32, true, SORTED>(R, e1, e0, ws, lane, A, B, DG, GORD, rec, PA, PB);
                    const unsigned c8 = merge_step<NR, W32, true, SORTED>(R, e0, e1, ws, lane, A, B, DG, GORD, rec, PA, PB);
                    const unsigned c9 = merge_step<NR, W32, true, SORTED>(R, e1, e0, ws, lane, A, B, DG, GORD, rec, PA, PB);
                    put5(c5, c6, c7, c8, c9);
                }
                if (it < nloop) {   // G*G not a multiple of 10: the remaining steps, one at a time
                    unsigned long long word = 0;
                    int k = 0;
                    for (int par = 0; it < nloop; ++it, par ^= 1) {
                        const unsigned long long c = par ? merge_step<NR, W32, true, SORTED>(R, e1, e0, ws, lane, A, B, DG, GORD, rec, PA, PB)
                                                         : merge_step<NR, W32, true, SORTED>(R, e0, e1, ws, lane, A, B, DG, GORD, rec, PA, PB);
                        word |= c << (12 * k);
                        if (++k == kCodesPerWord) { *pw = word; pw += kWave; word = 0; k = 0; }
                    }
                    if (k) *pw = word;
                }
                // ---- resolve the bins: merged k -> ASAVE, (frac, 1/sum, weight) -> rec rows 0-2 -------------------
                double ck = 0.0, cs = 0.0;
                const int ig = walk_bins(ws, GORD);
                constexpr int kRB = 5;
                for (int b0 = 0; b0 < G; b0 += kRB) {
                    double rka[kRB], rs1[kRB], rgd[kRB];
                    unsigned rcd[kRB];
#pragma unroll
                    for (int k = 0; k < kRB; ++k) {
                        const int bi = (b0 + k < G) ? b0 + k : G - 1;
                        const unsigned ro = (unsigned)bi * kRecBin + (unsigned)lane * 16u;
                        const dbl2 v0 = gld<dbl2>(rec, ro), v1 = gld<dbl2>(rec, ro + kRecRow);
                        rka[k] = v0.x; rs1[k] = v0.y; rgd[k] = v1.x; rcd[k] = (unsigned)__double_as_longlong(v1.y);
                    }
#pragma unroll
                    for (int k = 0; k < kRB; ++k) {
                        const int b = b0 + k;
                        if (b < G) {
                            double outv = 0.0, fr = 0.0, rinv = 1.0, w = 0.0;
                            if (b < ig) {
                                // the closing element, re-formed from LDS as the walk formed it
                                const int crow = rcd[k] & 31, ccol = (rcd[k] >> 5) & 63;
                                const double cv = A[crow * kWave + lane] + B[ccol * kWave + lane];
                                if constexpr (SORTED) w = pair_weight<W32>(DG, crow, ccol);
                                else w = pair_weight<W32>(DG, PA[crow * kWave + lane], PB[ccol * kWave + lane]);
                                const double ka = rka[k], s1 = rs1[k], cw = cv * w, gd0 = rgd[k];
                                const double gprev = (b == 0 && s1 == 0.0) ? wtot : gd0;
                                const double gdn = gd0 + w;
                                fr = fast_div(GORD[b + 1] - gprev, gdn - gprev);
                                const double kb = (ck + ka) + fr * cw;
                                const double sb = (cs + s1) + fr * w;
                                rinv = fast_div(1.0, sb);
                                outv = fast_div(kb, sb);
                                ck = (1.0 - fr) * cw;
                                cs = (1.0 - fr) * w;
                            } else if (b == ig) {
                                const double kb = ck + ws.kacc, sb = cs + ws.sum1;
                                if (b == G - 1) { outv = fast_div(kb, sb); rinv = fast_div(1.0, sb); } else outv = kb;
                            }
                            const unsigned ro = (unsigned)b * kRecBin + (unsigned)lane * 16u;
                            ASAVE[b * kWave + lane] = outv;
                            // what the replay passes read: (frac | row, column of the closing element; 1 / weight-sum)
                            const double frc = __longlong_as_double((__double_as_longlong(fr) & ~0x7FFLL) | (long long)(rcd[k] & 0x7FFu));
                            gst<dbl2>(rec, ro, dbl2{frc, rinv});
                        }
                    }
                }
                // ---- replay, one gathered vector per pass: the vector in A, bin sums in B (G+1 rows) ---------
                auto stage_row = [&](const double *src) {
                    if constexpr (SORTED) stage_slice(A, src, G, lane); else stage_slice_perm(A, src, PA, G, lane);
                };
                auto stage_col = [&](const double *src) {
                    if constexpr (SORTED) stage_slice(A, src, G, lane); else stage_slice_perm(A, src, PB, G, lane);
                };
                if (pg.gas_mask >> 31) {   // temperature slot: D_old[igas+1][row] + dkdT_new[col]*amount, as a row pass plus a column pass
                    double *DT = Dnew + (size_t)(igas + 2) * GW;
                    stage_row(Dold + (size_t)(igas + 1) * GW);
                    double tail = grad_replay<false, W32, SORTED>(nloop, lane, perm, A, B, DG, PA, PB);
                    grad_resolve<false, false, W32, SORTED>(G, lane, ig, rec, A, B, tail, DT, DG, PA, PB);
                    stage_col(DTB);
                    tail = grad_replay<true, W32, SORTED>(nloop, lane, perm, A, B, DG, PA, PB);
                    grad_resolve<true, true, W32, SORTED>(G, lane, ig, rec, A, B, tail, DT, DG, PA, PB);
                }
                if ((pg.gas_mask >> (igas + 1)) & 1u) {   // the new gas's slot: k_new[col]
                    stage_col(KRB);
                    const double tail = grad_replay<true, W32, SORTED>(nloop, lane, perm, A, B, DG, PA, PB);
                    grad_resolve<true, false, W32, SORTED>(G, lane, ig, rec, A, B, tail, Dnew + (size_t)(igas + 1) * GW, DG, PA, PB);
                }
                for (int pp = 0; pp <= igas; ++pp) {   // earlier gases: D_old[pp][row]
                    if (!((pg.gas_mask >> pp) & 1u)) continue;
                    stage_row(Dold + (size_t)pp * GW);
                    const double tail = grad_replay<false, W32, SORTED>(nloop, lane, perm, A, B, DG, PA, PB);
                    grad_resolve<false, false, W32, SORTED>(G, lane, ig, rec, A, B, tail, Dnew + (size_t)pp * GW, DG, PA, PB);
                }
                for (int pp = n; pp < NP1; ++pp)
                    for (int g = 0; g < G; ++g) Dnew[(size_t)pp * GW + g * kWave + lane] = 0.0;
                stage_slice(A, ASAVE, G, lane);
                if constexpr (!SORTED) {   // the merged spectrum is ascending with the plain del_g weights
                    for (int g = 0; g < G; ++g) PA[g * kWave + lane] = (unsigned char)g;
                    alast = A[(G - 1) * kWave + lane];
                }
            }
            cur ^= 1;
        }
        double *out = p.tau + (((size_t)m * p.L + l) * G) * p.Wpad + nu;
        if constexpr (SORTED) {
            if (unsorted) atomicOr(p.err_flag, 1);
            for (int g = 0; g < G; ++g) out[(size_t)g * p.Wpad] = A[g * kWave + lane];
        } else {
            for (int g = 0; g < G; ++g) out[(size_t)PA[g * kWave + lane] * p.Wpad] = A[g * kWave + lane];
        }
        double *dout = pg.dk + (((size_t)m * p.L + l) * NP1) * G * p.Wpad + nu;
        const double *Dc = gs + (cur ? dboff[1] : dboff[0]);
        for (int pp = 0; pp < NP1; ++pp) {
            const bool wanted = ((pg.gas_mask >> (pp == NP1 - 1 ? 31 : pp)) & 1u) != 0;
            for (int g = 0; g < G; ++g)
                dout[((size_t)pp * G + g) * p.Wpad] = wanted ? Dc[(size_t)pp * GW + g * kWave + lane] : 0.0;
        }
    }
}

}  // namespace ansfm

// ansfm_overlap_kernels.hip.h -- k_ck_overlap, the forward merge kernel of the correlated-k path (unit: ansfm_overlap.hip).
#pragma once
#include "ansfm_merge64.hip.h"

namespace ansfm {

// ------------------------------------------------------------------------------------------------
// K1+K2 fused: (P,T) interpolation + random-overlap merge.   "ck_overlap"
//
// One LANE per (wavenumber, layer) cell; a wavefront = 64 consecutive wavenumbers of ONE layer, so
// corner indices, u, v and gas amounts are wave-uniform (SGPRs) and every table access is one
// 512-byte coalesced row.  (The fast path, OPT != 0, can instead take 1 or kLaneNV wavenumbers x 64 or 64 / kLaneNV rows per wave,
// bit 0 of the argument flags, the argument lane_nv and LaneRow in ansfm_merge_common.hip.h: the merge below does not care which cell a lane holds.)
// The reference sorts the G*G sums tau_i + k_j*amount (argsort) and walks the sorted list once to re-bin it (rank, ForwardModel_0.py:6117-6173).  Both inputs are
// already sorted in g, so the sorted sequence is produced by a G-way streaming merge of the rows
// (a_i + b_0..b_{G-1}) -- the row heads held as a sorted list in registers, see merge_step -- and rank's walk
// consumes it on the fly: nothing of size G*G is ever stored.  The per-lane arrays a[G], b[G+1] live in LDS as
// [index][lane], so a lane-dependent index never causes a bank conflict (bank depends on the lane only).
//
// LDS per wave: (2G+1)*64*8 bytes (+ shared del_g / g_ord tables)  -> 21.1 KiB at G=20, 7 waves per CU.
// ------------------------------------------------------------------------------------------------

// SORTED = false: generic path for k-distributions that are not non-decreasing in g (the reference sorts the G*G
// products itself, :6150).  Each gas's (k, weight) pairs are sorted per lane first -- the multiset of
// (product, weight) is unchanged, so rank()'s walk sees the same sequence up to the order of exact ties -- and the
// skip rules keep looking at the LAST g-ordinate in the original order (:6075-6102).  A spectrum that passes through
// unmerged comes out in its original order.
// NOBOX: the table was found free of boxed entries at upload, load_gas interpolates without the box tests.
// OPT: 0, or the division-free fast path's kOptBfi | kOptExit | kOptOrient with or without kOptTable (ansfm_merge64.hip.h).  With kOptTable the
// launch is ONE BLOCK OF SEVERAL WAVES PER CU (as many as the LDS holds, blockDim.x / 64) that share DG / GORD and the weight
// product table WT; rows, tile queue, bin records and the sentinel row stay per wave and there is no barrier after the one
// that publishes the tables, so the waves run and leave independently as the one-wave blocks do.  With kOptOrient a wave's
// rows are a[G], a "huge" row, b[G], a "huge" row (merge_wave_rows): column G of either operand is a sentinel.
// Gas s of the cell a lane holds, in either mapping: the lane's own row (fast path with lane_rows) or row (m, l) of the wave
template <bool FROM_K, bool NOBOX, int OPT>
__device__ __forceinline__ void load_cell(const OverlapParams &p, int lane_rows, bool gfast, const LaneRow &lr, const LayerInterp &q, int m,
                                          int l, int s, int nu, double *DST, int lane, bool &unsorted)
{
    if constexpr (OPT != 0) {
        if (lane_rows != 0) {
            if (!FROM_K && gfast) load_gas_rows<FROM_K, NOBOX, true>(p, lr, s, DST, lane, unsorted);
            else load_gas_rows<FROM_K, NOBOX, false>(p, lr, s, DST, lane, unsorted);
            return;
        }
    }
    load_gas<FROM_K, false, NOBOX>(p, q, m, l, s, nu, DST, lane, unsorted);
}

template <int NR, bool FROM_K, bool W32, bool SORTED = true, bool NODIV = false, bool NOBOX = false, int OPT = 0>
__global__ __launch_bounds__((OPT & kOptTable) != 0 ? kWave * kMaxBlockWaves : kWave) __attribute__((amdgpu_waves_per_eu(1, 2)))
void k_ck_overlap(OverlapParams p, int flags, int lane_nv)
{
    static_assert(OPT == 0 || (SORTED && NODIV), "the fast path");
    static_assert(merge_opt_valid(OPT), "OPT == 0 || (OPT & ~kOptTable) == (kOptBfi | kOptExit | kOptOrient)");
    constexpr bool kTable = (OPT & kOptTable) != 0, kOrient = (OPT & kOptOrient) != 0;
    static_assert(!kTable || W32, "the weight table holds float32 products only (launch_overlap)");
    // the table kernels of the lists from kSuffixMinList entries carry the partial form of the walk (merge_suffix_row); the shorter
    // ones take a merge whole or not at all, with the test and the code they had
    constexpr bool kSuffix = kTable && NR >= kSuffixMinList;
    // the table kernels of the lists from kStaticMinList entries carry the static schedule of a whole walk and the reciprocal table
    // (flags bit kFlagStatic: the launch has a valid schedule and the block its tables; kFlagStaticOff: the walk steps per lane)
    constexpr bool kStatic = kTable && NR >= kStaticMinList;
    const bool st_tables = kStatic && (flags & kFlagStatic) != 0;
    const bool st_walk = kStatic && (flags & (kFlagStatic | kFlagStaticOff)) == kFlagStatic;
    // flags: the row mapping (kFlagLaneRows) and, with kOptTable only, the list-free walk of row-major merges (kFlagRowMajor) and
    // "no walk of the top rows of a list merge" (kFlagSuffixOff);
    // the instantiations without the table are launched with 0 or 1 and test the word as they always did
    // (lane_rows is only ever compared with 0, and kFlagTableGfast is set only together with kFlagLaneRows)
    const int lane_rows = kTable ? (flags & kFlagLaneRows) : flags;
    // the table is read from its g-fastest copy: table launches of the row mapping only
    const bool gfast = !FROM_K && OPT != 0 && (flags & kFlagTableGfast) != 0;
    // lane_nv: the wavenumbers of a tile of the row mapping, 1 or kLaneNV (LaneRow); unused without lane_rows
    const unsigned nvs = lane_nv == 1 ? 0u : kLaneNVShift;
    unsigned n_rowmajor = 0, n_merged = 0;              // kOptTable: the merges of this wave that took the walk / all of them
    unsigned n_suffix = 0;                              // kOptTable: the rows this wave walked behind a list phase
    unsigned n_static = 0;                              // kStatic: the merges of this wave walked on the static schedule
    // kOptTable: the launch orders a block's wavenumbers by the launch before's pattern bytes and writes its own (MergePlan::order)
    const bool ordered = kTable && p.hint_in != nullptr;
    unsigned n_hints = 0;                               // the non-zero pattern bytes this wave read for the blocks whose tile 0 it ran
    extern __shared__ double smem[];
    const int lane = kTable ? (int)(threadIdx.x & 63u) : (int)threadIdx.x;
    const int wv = kTable ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : 0;     // wave of the block
    const int nwv = kTable ? (int)(blockDim.x >> 6) : 1;
    const int G = p.G;
    // tables first: their LDS addresses are compile-time constants (dynamic LDS starts at 0), so a table read is
    // `ds_read vaddr = index << k, offset:const` with no base add
    double *DG = smem;                           // [kMaxG] doubles, then GORD [kMaxG + 2], then the float32 copy of DG
    double *GORD = DG + kMaxG;
    double *A = reinterpret_cast<double *>(reinterpret_cast<char *>(GORD + kMaxG + 2) + kMaxG * sizeof(float));
    if constexpr (kTable) {
        // WT[(col << 5) | row] = the very double pair_weight<true> forms (DGF[i] = (float)del_g[i]); 0 outside
        double *WT = A;
        for (int idx = (int)threadIdx.x; idx < (G + 1) * 32; idx += (int)blockDim.x) {
            const int row = idx & 31, col = idx >> 5;
            double w = 0.0;
            if (row < G && col < G) w = (double)((float)p.del_g[row] * (float)p.del_g[col]);
            WT[idx] = w;
        }
        A = WT + (G + 1) * 32 + (size_t)wv * merge_wave_rows(G, OPT) * kWave;
        if constexpr (kStatic) {
            if (st_tables) {
                A += kMergeStaticLds / sizeof(double);
                if (wv == 0) merge_static_fill(p, G, lane);
            }
        }
    }
    double *B = A + (kOrient ? G + 1 : G) * kWave;   // G+1 rows
    unsigned char *PA = reinterpret_cast<unsigned char *>(B + (G + 1) * kWave);   // SORTED = false only
    unsigned char *PB = PA + G * kWave;
    if (wv == 0 && lane < G) {
        DG[lane] = p.del_g[lane];
        const_cast<float *>(delg_f32_table(DG))[lane] = (float)p.del_g[lane];
    }
    if (wv == 0 && lane < G + 2) GORD[lane] = p.g_ord[lane];
    const double HUGE_KEY = __longlong_as_double(0x7FE0000000000000LL);   // finite, above any optical depth
    B[G * kWave + lane] = HUGE_KEY;
    if constexpr (kOrient) A[G * kWave + lane] = HUGE_KEY;
    __syncthreads();
    double wsum = 0.0;
    for (int g = 0; g < G; ++g) wsum += DG[g];
    const double wtot = wsum * wsum;  // stands in for gdist[-1] (python wrap at iloop==0)

    // per-block scratch: closed-bin records, see kRecBin
    double *rec = p.scratch + ((size_t)blockIdx.x * nwv + wv) * 6 * G * kWave;
    TileQueue tq;
    tq.init();
    for (;;) {
        int vt = 0, m = 0, l = 0;
        LaneRow lr{};                                   // layer-grouped lanes (OPT != 0 and lane_rows): the lane's own row
        if constexpr (OPT != 0) {
            if (lane_rows != 0) {
                unsigned k = 0;
                if (!tq.next_rows(p, lane, nvs, vt, k)) break;
                if constexpr (kTable) {
                    int inv = lane;
                    if (ordered) {
                        bool nonzero = false;
                        inv = merge_order_inverse(p.hint_in, vt, p.W, lane, nonzero);
                        if (k == 0) n_hints += (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(nonzero));
                    }
                    lr = lane_row<FROM_K>(p, vt, k, lane, nvs, gfast, ordered, inv);
                } else
                lr = lane_row<FROM_K>(p, vt, k, lane, nvs, gfast);
            } else if (!tq.next(p, lane, vt, m, l)) break;
        } else {
            if (!tq.next(p, lane, vt, m, l)) break;
        }
        const int nu = vt * kWave + lane;
        LayerInterp q;
        if constexpr (!FROM_K) q = p.li[(size_t)m * p.L + l];
        bool unsorted = false;
        unsigned pattern = 0;                           // ordered: the lane's verdicts of merges 1 .. 8, merge 1 in bit 7

        load_cell<FROM_K, NOBOX, OPT>(p, lane_rows, gfast, lr, q, m, l, 0, nu, A, lane, unsorted);
        double alast = A[(G - 1) * kWave + lane];       // last g-ordinate in the ORIGINAL order
        if constexpr (!SORTED) sort_column(A, PA, G, lane);
        for (int s = 1; s < p.S; ++s) {
            load_cell<FROM_K, NOBOX, OPT>(p, lane_rows, gfast, lr, q, m, l, s, nu, B, lane, unsorted);
            if constexpr (SORTED)                       // the call is rerun on the generic path: no point in merging
                if (__builtin_amdgcn_ballot_w64(unsorted) != 0) break;
            const double blast = B[(G - 1) * kWave + lane];
            if constexpr (!SORTED) sort_column(B, PB, G, lane);
            if constexpr (SORTED) alast = A[(G - 1) * kWave + lane];
            // skip rules, cutoff = 0  (ForwardModel_0.py:6073-6102)
            bool takeB, keepA;
            if (s == 1) { takeB = (alast <= 0.0); keepA = !takeB && (blast <= 0.0); }
            else { keepA = (blast <= 0.0); takeB = !keepA && (alast <= 0.0); }
            const bool do_merge = !(takeB | keepA);
            bool walked = false;                        // kOptTable: the merge was walked row by row (wave-uniform where set)
            bool walked_static = false;                 // kStatic: ... and on the static schedule
            int walked_rows = 0;                        // kOptTable: its rows walked behind a list phase (the same in every merging lane)
            if (takeB) {
                for (int g = 0; g < G; ++g) A[g * kWave + lane] = B[g * kWave + lane];
                if constexpr (!SORTED) {
                    for (int g = 0; g < G; ++g) PA[g * kWave + lane] = PB[g * kWave + lane];
                    alast = blast;
                }
            }
            if (do_merge) {
                // ---- sorted list of the G row heads (row i = a_i + b_j, j ascending) -------------
                double R[NR];
                MergeOrient mo{};
                if constexpr (kOrient) {
                    // rows = the operand with the larger top ordinate; b can be the rows only where a ascends (MergeOrient)
                    bool swapped = blast > alast;
                    if (__builtin_amdgcn_ballot_w64(swapped) != 0) {
                        double prev = A[lane];
                        for (int g = 1; g < G; ++g) {
                            const double v = A[g * kWave + lane];
                            swapped &= (v >= prev);
                            prev = v;
                        }
                    }
                    mo = merge_orient(lds_addr(A + lane), lds_addr(B + lane), swapped);
                    merge_init<NR>(R, G, mo, HUGE_KEY);
                } else
                    merge_init<NR>(R, G, lane, A, B[lane], HUGE_KEY);
                // (declared in this order on purpose: with the walk state first the compiler commutes operands of the walk in
                // every instantiation -- same results, other instructions)
                MergeElem e0, e1;
                WalkState ws;
                int i0 = G;                             // kOptTable: the row from which the merge is walked (merge_suffix_row)
                if constexpr (kTable) {
                    bool lane_passes = false;
                    if constexpr (kSuffix) {
                        if ((flags & kFlagRowMajor) != 0)
                            i0 = merge_suffix_row(merge_rowmajor_test<NR>(R, G, mo, lane_passes), G, (flags & kFlagSuffixOff) == 0);
                    } else {
                        if ((flags & kFlagRowMajor) != 0 && merge_rowmajor_whole<NR>(R, G, mo, lane_passes)) i0 = 0;
                    }
                    walked = i0 == 0;
                    if (i0 != 0) walked_rows = G - i0;
                    // (a skipped merge leaves its bit 0; merges beyond the eighth shift their bit out)
                    pattern |= lane_passes && s <= 8 ? 0x100u >> s : 0u;
                }
                if (!kTable || i0 != 0) {               // (a constant without the table: those instantiations compile as they did)
                merge_fetch<W32, SORTED, OPT>(R[0], lane, A, B, DG, e0, PA, PB, mo);
                ws = walk_begin(GORD, lane);
                // full-length passes for the steps 0 .. G*G - G (an odd number of them), then the peeled ones (merge_peel);
                // kOptTable, a list phase below the rows that are walked: G * i0 full-length passes, odd or even, and no peel --
                // the heads of the rows from i0 stay at the tail of R, and the element the last step fetched is theirs
                const bool partial = kSuffix && i0 < G;
                const int nloop = partial ? G * i0 : G * G - (G - 1);
                // ping-pong: no register rotation.  The trips are counted down (one scalar add and one compare per trip)
                // (kPer is a named local on purpose: with a literal 2 the compiler orders the scalar code of the skip rules
                // above differently in the OPT = 0 instantiations -- same results, other instructions)
                constexpr int kPer = 2;         // steps per trip
                for (int n = nloop / kPer; n > 0; --n) {
                    merge_step<NR, W32, false, SORTED, NODIV, NR, OPT>(R, e0, e1, ws, lane, A, B, DG, GORD, rec, PA, PB, mo);
                    merge_step<NR, W32, false, SORTED, NODIV, NR, OPT>(R, e1, e0, ws, lane, A, B, DG, GORD, rec, PA, PB, mo);
                }
                if (!partial || (nloop & 1) != 0)
                merge_step<NR, W32, false, SORTED, NODIV, NR, OPT>(R, e0, e1, ws, lane, A, B, DG, GORD, rec, PA, PB, mo);
                if (!partial) {
                if (((G ^ NR) & 1) != 0) { const MergeElem t = e0; e0 = e1; e1 = t; }   // current element: e1 <-> e0
                merge_peel<NR - 1, NR, W32, SORTED, NODIV, OPT>(R, e0, e1, ws, G, lane, A, B, DG, GORD, rec, PA, PB, mo);
                }
                }
                if constexpr (kTable) {
                    // the one call of the walk: the whole merge, or the rows behind a list phase, on the same walk state
                    if (i0 < G) {
                        if constexpr (kStatic) walked_static = i0 == 0 && st_walk;
                        if (!walked_static) {
                            if (i0 == 0) ws = walk_begin(GORD, lane);
                            merge_rowmajor<NR>(i0, G, mo, ws, rec);
                        }
                    }
                }
                if constexpr (kStatic) {
                if (walked_static) {
                    // ---- the whole walk on the schedule: closed sums into A's slots, divided in place; the open bin as below ----
                    const unsigned a_lane = lds_addr(A + lane), sb = merge_static_base(G);
                    const double kacc = merge_rowmajor_static<NR>(G, mo, a_lane);
                    const int ig = p.st.nbins;
                    for (int g0 = 0; g0 < G; g0 += kLoadBatch) {
                        double r[kLoadBatch];
                        dbl2 rd[kLoadBatch];
#pragma unroll
                        for (int k = 0; k < kLoadBatch; ++k) {
                            const unsigned b = (unsigned)((g0 + k < G) ? g0 + k : G - 1);
                            r[k] = lds_ld(a_lane + b * 512u);
                            rd[k] = lds_ld2(sb + kStaticRD + b * 16u);
                        }
#pragma unroll
                        for (int k = 0; k < kLoadBatch; ++k) {
                            const int b = g0 + k;
                            if (b < G) {
                                double outv = 0.0;
                                if (b < ig) outv = recip_div(r[k], rd[k]);
                                else if (b == ig) outv = (b == G - 1) ? fast_div(kacc, p.st.last_width) : kacc;
                                A[b * kWave + lane] = outv;
                            }
                        }
                    }
                }
                }
                if (!walked_static) {
                if constexpr (NODIV) {
                    // ---- normalise: closed bins by their width; the open one as rank()'s trailing `if ig == ng-1` (:6171) ----
                    const int ig = walk_bins(ws, GORD);
                    for (int g0 = 0; g0 < G; g0 += kLoadBatch) {
                        double r[kLoadBatch];
#pragma unroll
                        for (int k = 0; k < kLoadBatch; ++k)
                            r[k] = gld<double>(rec, (unsigned)((g0 + k < G) ? g0 + k : G - 1) * (kWave * 8u) + (unsigned)lane * 8u);
#pragma unroll
                        for (int k = 0; k < kLoadBatch; ++k) {
                            const int b = g0 + k;
                            if (b < G) {
                                double outv = 0.0;
                                if (b < ig) {
                                    // the width's reciprocal once per block where the launch carries the table: the same quotient
                                    if (st_tables) outv = recip_div(r[k], lds_ld2(merge_static_base(G) + kStaticRD + (unsigned)b * 16u));
                                    else outv = fast_div(r[k], GORD[b + 1] - GORD[b]);
                                }
                                else if (b == ig) outv = (b == G - 1) ? fast_div(ws.kacc, ws.gd - GORD[G - 1]) : ws.kacc;
                                A[b * kWave + lane] = outv;
                            }
                        }
                    }
                } else {
                // ---- resolve the bins --------------------------------------------------------------------
                // The closing element of every bin is re-formed from LDS (a[row] + b[col], its weight) exactly as the
                // walk formed it, so `a` must stay intact until the last bin is done: the outputs go to row 0 of the bin
                // records (full-wave coalesced stores) and come back into A afterwards.
                double ck = 0.0, cs = 0.0;   // (1-frac) share carried into the next bin
                const int ig = walk_bins(ws, GORD);
                constexpr int kRB = 5;       // records of kRB bins are fetched together (one round trip)
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
                            double outv = 0.0;
                            if (b < ig) {
                                const int crow = rcd[k] & 31, ccol = (rcd[k] >> 5) & 63;
                                const double cv = A[crow * kWave + lane] + B[ccol * kWave + lane];
                                double w;
                                if constexpr (SORTED) w = pair_weight<W32>(DG, crow, ccol);
                                else w = pair_weight<W32>(DG, PA[crow * kWave + lane], PB[ccol * kWave + lane]);
                                const double ka = rka[k], s1 = rs1[k], cw = cv * w;
                                // a crossing at the very first element (nothing accumulated yet) sees python's gdist[-1]
                                const double gd0 = rgd[k];
                                const double gprev = (b == 0 && s1 == 0.0) ? wtot : gd0;
                                const double gdn = gd0 + w;                 // the same add the walk made
                                const double frac = fast_div(GORD[b + 1] - gprev, gdn - gprev);     // <= 1 ulp, as every division of the resolve
                                const double kb = (ck + ka) + frac * cw;
                                const double sb = (cs + s1) + frac * w;
                                outv = fast_div(kb, sb);
                                ck = (1.0 - frac) * cw;
                                cs = (1.0 - frac) * w;
                            } else if (b == ig) {
                                // trailing `if ig == ng-1` (:6171); an unfinished earlier bin stays un-normalised
                                const double kb = ck + ws.kacc, sb = cs + ws.sum1;
                                outv = (b == G - 1) ? fast_div(kb, sb) : kb;
                            }
                            gst<double>(rec, (unsigned)b * kRecBin + (unsigned)lane * 16u, outv);
                        }
                    }
                }
                for (int g0 = 0; g0 < G; g0 += kLoadBatch) {          // merged spectrum: records' row 0 -> A
                    double r[kLoadBatch];
#pragma unroll
                    for (int k = 0; k < kLoadBatch; ++k)
                        r[k] = gld<double>(rec, (unsigned)((g0 + k < G) ? g0 + k : G - 1) * kRecBin + (unsigned)lane * 16u);
#pragma unroll
                    for (int k = 0; k < kLoadBatch; ++k)
                        if (g0 + k < G) A[(g0 + k) * kWave + lane] = r[k];
                }
                }
                }
                if constexpr (!SORTED) {   // the merged spectrum is ascending with the plain del_g weights
                    for (int g = 0; g < G; ++g) PA[g * kWave + lane] = (unsigned char)g;
                    alast = A[(G - 1) * kWave + lane];
                }
            }
            if constexpr (kTable) {
                n_merged += __builtin_amdgcn_ballot_w64(do_merge) != 0 ? 1u : 0u;
                n_rowmajor += __builtin_amdgcn_ballot_w64(walked) != 0 ? 1u : 0u;
                if constexpr (kStatic) n_static += __builtin_amdgcn_ballot_w64(walked_static) != 0 ? 1u : 0u;
                // (counted here, where every lane is active: lane 0, which adds the totals up, need not have merged)
                const unsigned long long some = __builtin_amdgcn_ballot_w64(walked_rows != 0);
                if (some != 0) n_suffix += (unsigned)__builtin_amdgcn_readlane(walked_rows, __builtin_ctzll(some));
            }
        }
        if constexpr (OPT != 0) {
            if (lane_rows != 0) {                     // the lane's own row of tau[n][L][G][Wpad]
                if (unsorted) atomicOr(p.err_flag, 1);
                double *outr = p.tau + ((size_t)lr.row * G) * p.Wpad + lr.nu;
                for (int g = 0; g < G; ++g) outr[(size_t)g * p.Wpad] = A[g * kWave + lane];
                if constexpr (kTable) {
                    // every cell is in exactly one tile: the wavenumber's byte is written once per launch, by its middle row
                    if (ordered && lr.row == (((unsigned)p.n_models * (unsigned)p.L) >> 1) && lr.nu < p.W)
                        p.hint_out[lr.nu] = (unsigned char)pattern;
                }
                continue;
            }
        }
        double *out = p.tau + (((size_t)m * p.L + l) * G) * p.Wpad + nu;
        if constexpr (SORTED) {
            if (unsorted) atomicOr(p.err_flag, 1);
            for (int g = 0; g < G; ++g) out[(size_t)g * p.Wpad] = A[g * kWave + lane];
        } else {
            for (int g = 0; g < G; ++g) out[(size_t)PA[g * kWave + lane] * p.Wpad] = A[g * kWave + lane];
        }
    }
    if constexpr (kTable) {
        // the launch's five totals follow the tile counters (merge_params) and are cleared with them; added once per wave
        unsigned long long *cnt = reinterpret_cast<unsigned long long *>(p.tile_counter + 8);
        if (lane == 0) {
            atomicAdd(cnt, (unsigned long long)n_rowmajor);
            atomicAdd(cnt + 1, (unsigned long long)n_merged);
            if (ordered) atomicAdd(cnt + 2, (unsigned long long)n_hints);
            if (n_suffix != 0) atomicAdd(cnt + 3, (unsigned long long)n_suffix);
            if (n_static != 0) atomicAdd(cnt + 4, (unsigned long long)n_static);
        }
    }
}

}  // namespace ansfm

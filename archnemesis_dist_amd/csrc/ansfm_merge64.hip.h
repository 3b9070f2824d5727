// ansfm_merge64.hip.h -- device code of the 64-bit-key merge that the forward kernel (ansfm_overlap_kernels.hip.h) and the
// gradient kernel (ansfm_overlapg_kernels.hip.h) share: the LDS layout, the list keys, the rank walk, the register-list step
// with its peeled tail, and the per-lane sort of the generic path.  No kernel is defined here, so both units include it.
//
// The code comes in two forms, chosen by the template parameter OPT of merge_fetch / merge_step / merge_peel:
//   OPT = 0   the plain form: the weight from its two factors, the key packed field by field, a full list pass per step.  The
//             gradient kernel, the generic (SORTED = false) and the recorded (NODIV = false) forward paths and
//             ANSFM_MERGE_LEGACY=1 run it.
//   OPT != 0  the division-free fast path of the forward kernel (SORTED, NODIV).  Three things that only pay together: the
//             popped row's next key is the winner's low word + 1 column inserted under the 11-bit mask (kOptBfi), the list
//             pass of a step ends at the first chunk boundary that no lane's key reaches beyond (kOptExit, merge_pass_exit),
//             and per lane and merge the rows are the operand with the larger top ordinate, so that the next key re-enters
//             near the front of the list (kOptOrient, MergeOrient).  With float32 weights the pair weight is in addition one
//             ds_read_b64 of a product table WT[(col << 5) | row] that the waves of one block per CU share (kOptTable); with
//             float64 weights the walk's gd + DG[i] * DG[j] is compiled as one fma, which no table of products reproduces.
//             With the table, a wave whose lanes' merges all sort row by row walks them without the list (merge_rowmajor), and
//             from the start of a merge on the launch's static schedule of bin crossings (merge_rowmajor_static).
// Both forms give the same results bit for bit (tests/test_merge_*.py).  What each piece bought, and the variants that were
// measured and lost (tools/experiments/r07_merge_retired_variants.patch), is in DESIGN.md section 4.1.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ansfm_merge_common.hip.h"

namespace ansfm {

// LDS byte offsets of the tables that open the merge kernels' dynamic LDS block (the kernels have no static LDS, so the
// block starts at address 0 -- checked once per launch): reads become `ds_read vaddr = index << k, offset:const`.
constexpr unsigned kLdsDG = 0, kLdsGORD = kMaxG * 8, kLdsDGF = (2 * kMaxG + 2) * 8, kLdsA = kLdsDGF + kMaxG * 4;

// One popped element of the merge with everything the rank walk and the row's next key need, fetched from LDS
// as soon as the winner key is known (software pipelining: the walk of element t and the rest of the insertion
// pass run while the operands of element t+1 are in flight).
// Bin records, per block [bin][2][lane] pairs of doubles: pair 0 = (kacc, sum1), pair 1 = (gd, code of the element that
// closed the bin: row | column << 5), each pair one 16-byte store per lane, the lanes of a pair contiguous (1 KiB rows).
// The stores sit in the merge loop's crossing branch, which runs in about every second step, and every store
// traffic there is not free (doubling five 8-byte row stores: +29 % on the forward kernel) -- so the closing element's
// value and weight are not stored, the resolve loop recomputes them from LDS (same operations), and what is stored goes
// out as two wide stores.  Same-box comparisons: gradient kernel 25.7 -> 23.7 ms against six 8-byte rows; forward kernel
// within +-1 % of five 8-byte rows and of three pairs (it is not store-bound at this level).  The gradient kernel's resolve rewrites the
// pairs as (frac, 1/weight-sum) and (weight, code) for its replay passes.

// The bits of OPT (kOpt*, kMergeOpt, merge_opt_valid), the launch flags (kFlag*), the rows per wave (merge_wave_rows) and the
// weight table's size (weight_table_bytes, kMaxBlockWaves) are in ansfm_merge_plan.h, where the launcher's plan reads them too.
// The product table follows the float32 copy of DG; the per-wave rows come after it.
constexpr unsigned kLdsWT = kLdsA;
static_assert(kLdsA == kMergeLdsTables, "the plan's LDS arithmetic");
typedef double dbl2 __attribute__((ext_vector_type(2)));
constexpr unsigned kRecRow = 64u * 16u, kRecBin = 2u * kRecRow;

struct MergeElem {
    double ai, bc, bn, w;
    int ci, np;         // np = column + 1; on the fast path the winner key's low word instead (the fetch decodes ci and the column)
};

// kOptOrient: which operand supplies the rows is a per-lane choice, made once per merge.  The merge is symmetric in its operands
// (a_i + b_j, del_g[i] * del_g[j] as a float32 or float64 product), and with the larger operand as the rows the sorted order
// runs row by row: the popped row's next key re-enters the list near its front, where kOptExit ends the pass.  A lane whose
// rows are b ("swapped") needs its columns, a, ascending; a merged spectrum is that only up to rounding (merge_init), so such
// a lane is swapped only if its a is non-decreasing.  A swapped lane packs the low 11 key bits as (row << 6) | col instead of
// (col << 5) | row: both are (b-index major, a-index minor), so keys whose top 53 bits tie pop in the same order whichever
// way a lane is oriented, and the popped sequence of (a-index, b-index) pairs is the unswapped one's.  Rows stay below 32;
// the 6-bit column field holds the sentinel index G <= 32.
struct MergeOrient {
    unsigned rbase, cbase;  // LDS byte address of this lane's entry of row 0 / column 0
    unsigned rsh, csh;      // bit offset of the row / column field in the key's low word: 0, 5 or (swapped) 6, 0
    unsigned inc;           // column + 1 in the low word: 32 or (swapped) 1
};
__device__ __forceinline__ MergeOrient merge_orient(unsigned a_addr, unsigned b_addr, bool swapped)
{
    MergeOrient mo;
    mo.rbase = swapped ? b_addr : a_addr; mo.cbase = swapped ? a_addr : b_addr;
    mo.rsh = swapped ? 6u : 0u; mo.csh = swapped ? 0u : 5u; mo.inc = swapped ? 1u : 32u;
    return mo;
}

// Weight of element (i, j) = del_g[i] * del_g[j].  DELG float32 (W32): NumPy forms the float32 product, which is one
// v_mul_f32 of the float32 copies kept behind the double tables (DG, GORD) in LDS.
__device__ __forceinline__ const float *delg_f32_table(const double *DG) { return reinterpret_cast<const float *>(DG + 2 * kMaxG + 2); }
template <bool W32>
__device__ __forceinline__ double pair_weight(const double *DG, int i, int j)
{
    if constexpr (W32) {
        const float *DGF = delg_f32_table(DG);
        return (double)(DGF[i] * DGF[j]);
    } else
        return DG[i] * DG[j];
}

// SORTED = false (generic path): the rows / columns were sorted per lane beforehand; PA / PB give the original
// g-ordinate of each sorted position, which is the one whose weight applies.
template <bool W32, bool SORTED = true, int OPT = 0>
__device__ __forceinline__ void merge_fetch(double key, int lane, const double *A, const double *B,
                                            const double *DG, MergeElem &e,
                                            const unsigned char *PA = nullptr, const unsigned char *PB = nullptr,
                                            const MergeOrient &mo = MergeOrient{})
{
    static_assert(OPT == 0 || SORTED, "the fast path");
    static_assert(merge_opt_valid(OPT), "OPT == 0 || (OPT & ~kOptTable) == (kOptBfi | kOptExit | kOptOrient)");
    const unsigned kb = (unsigned)__double_as_longlong(key);
    if constexpr (OPT != 0) {
        // the fields at per-lane bit offsets, one instruction each, and the addresses on per-lane bases, so that every row
        // address is one v_lshl_add on top (the compiler otherwise forms (kw << k) & mask + base, three instructions).
        // The table index is formed from the decoded fields (WT is symmetric: the product of the two float32 weights)
        int ci, cp;
        asm("v_bfe_u32 %0, %1, %2, 5" : "=v"(ci) : "v"(kb), "v"(mo.rsh));
        asm("v_bfe_u32 %0, %1, %2, 6" : "=v"(cp) : "v"(kb), "v"(mo.csh));
        e.ci = ci;
        e.np = (int)kb;
        if constexpr ((OPT & kOptTable) != 0) e.w = lds_ld(kLdsWT + ((unsigned)cp << 8) + ((unsigned)ci << 3));
        e.ai = lds_ld(mo.rbase + ((unsigned)ci << 9));
        const unsigned ab = mo.cbase + ((unsigned)cp << 9);
        e.bc = lds_ld(ab);
        e.bn = lds_ld(ab + 512);                // column G of either operand is its sentinel row
        if constexpr ((OPT & kOptTable) == 0) e.w = pair_weight<W32>(DG, ci, cp);
    } else {
        const int ci = kb & 31, cp = (kb >> 5) & 63;
        e.ci = ci;
        e.np = cp + 1;
        e.ai = A[ci * kWave + lane];
        const unsigned ab = lds_addr(B + lane) + ((unsigned)cp << 9);
        e.bc = lds_ld(ab);
        e.bn = lds_ld(ab + 512);                // B[G] = sentinel column: an exhausted row re-enters as "huge"
        if constexpr (SORTED) e.w = pair_weight<W32>(DG, ci, cp);
        else e.w = pair_weight<W32>(DG, PA[ci * kWave + lane], PB[cp * kWave + lane]);
    }
}

// List keys: the element value a_i + b_j with the low 11 mantissa bits replaced by (col << 5) | row  (col <= 32,
// row <= 31).  Keys compare like the values except among values closer than 2^-41 relative (treated as ties, which
// rank() orders arbitrarily anyway); the exact value is recomputed from a_i + b_j when the element is consumed, so the
// sums are the reference's.
__device__ __forceinline__ double pack_key11(double v, int row, int col)
{
    unsigned long long b = (unsigned long long)__double_as_longlong(v);
    b = (b & ~0x7FFULL) | (unsigned long long)((col << 5) | row);
    return __longlong_as_double((long long)b);
}
// The next key of a popped row from the winner's low word kw = ... | col << 5 | row: col + 1 is kw + 32, and the 11 bits go
// into the value's low word under the mask (v_add_u32 + v_bfi_b32).  col <= 32, so the add does not leave the 11 bits for
// any key that is consumed; the same double as pack_key11(v, row, col + 1).
// inc: 32, or 1 in a lane whose key holds the column in its low six bits (MergeOrient; col + 1 <= 33 stays inside them).
__device__ __forceinline__ double pack_key11_next(double v, unsigned kw, unsigned inc)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = ((kw + inc) & 0x7FFu) | ((unsigned)b & ~0x7FFu);
    return __longlong_as_double((long long)((b & 0xFFFFFFFF00000000ULL) | lo));
}

// rank() walk state of one lane (ForwardModel_0.py:6155-6170).  Bin boundaries are recorded and resolved
// after the loop: frac needs a division, and the next bin's (1-frac) share is added there too -- the same
// sums in a different association.
struct WalkState {
    double gd, kacc, sum1, gnext;
    unsigned roff;      // byte offset of this lane's first pair in the record of the bin being filled: ig * kRecBin + lane * 16
    unsigned gaddr;     // LDS byte address of GORD[ig + 1]
    unsigned rbase;     // merge_walk_nodiv: lane * 8 - (address of GORD[1] << 6), see there (roff is unused in that walk)
};
__device__ __forceinline__ WalkState walk_begin(const double *GORD, int lane)
{
    WalkState ws;
    ws.gd = 0.0; ws.kacc = 0.0; ws.sum1 = 0.0;
    ws.gaddr = lds_addr(GORD + 1);
    ws.gnext = lds_ld(ws.gaddr);
    ws.roff = (unsigned)lane * 16u;
    ws.rbase = (unsigned)lane * 8u - (ws.gaddr << 6);
    return ws;
}
// number of bins closed so far
__device__ __forceinline__ int walk_bins(const WalkState &ws, const double *GORD)
{
    return (int)((ws.gaddr - lds_addr(GORD + 1)) >> 3);
}

template <bool REC_CODE>
__device__ __forceinline__ bool merge_walk(const MergeElem &e, WalkState &ws, double *rec, const double *GORD,
                                           int lane)
{
    const double cv = e.ai + e.bc;
    const double w = e.w;
    const double gdn = ws.gd + w;
    double kn = ws.kacc + cv * w, sn = ws.sum1 + w;
    // ordered >= : GORD[G+1] is NaN, so nothing crosses after the last bin whatever gdn is (garbage weights of a call
    // that is going to be rerun on the generic path, NaN / inf input) -- the record index stays <= G
    const bool cross = (gdn >= ws.gnext);
    if (cross) {                                // this element straddles the bin boundary
        // The branch runs in about every second step (some lane of the 64 crosses), so it is kept to four stores and two
        // adds: the record slot is a running 32-bit byte offset onto the wave-uniform base (no 64-bit index arithmetic).
        gst<dbl2>(rec, ws.roff, dbl2{ws.kacc, ws.sum1});
        gst<dbl2>(rec, ws.roff + kRecRow, dbl2{ws.gd, __longlong_as_double((long long)(e.ci | ((e.np - 1) << 5)))});
        kn = 0.0; sn = 0.0;
        ws.roff += kRecBin;
        ws.gaddr += 8u;
        ws.gnext = lds_ld(ws.gaddr);            // GORD[G+1] = NaN: nothing crosses after the last bin
    }
    ws.kacc = kn; ws.sum1 = sn;
    ws.gd = gdn;
    return cross;
}

// Division-free form of the walk (forward kernel, NODIV).  rank()'s boundary element contributes frac * cont * w to the bin
// it closes and (1 - frac) * cont * w to the next one, frac = (g_ord[ig+1] - gdist_prev) / w: that is
// (g_ord[ig+1] - gdist_prev) * cont and (gdist - g_ord[ig+1]) * cont -- no division -- and the bin's weight sum (carry
// (1-frac) w of the previous boundary element, the weights inside, frac w) telescopes to g_ord[ig+1] - g_ord[ig].  A closed
// bin is then ONE 8-byte store of its un-normalised sum (rec = [bin][lane] doubles) instead of a 32-byte record, and the
// resolve pass is a division by the bin width when the merged spectrum is read back.  Differs from the recorded form
// in the last bits only (the reference itself forms frac from a difference of cumulative sums, good to ~1e-12).
// Precondition (checked at launch): the first element of the merged order does not close a bin -- rank()'s python
// gdist[-1] wrap, which only the recorded form reproduces.
__device__ __forceinline__ bool merge_walk_nodiv(const MergeElem &e, WalkState &ws, double *rec)
{
    const double cv = e.ai + e.bc;
    const double w = e.w;
    const double gdn = ws.gd + w;
    double kn = fma(cv, w, ws.kacc);
    const bool cross = (gdn >= ws.gnext);       // ordered: GORD[G+1] is NaN
    if (cross) {
        // The closed bin's slot, ig * 512 + lane * 8, is formed from the one running offset the walk keeps (gaddr, +8 per
        // bin; 512 = 8 << 6): one shift-add here, where a second running offset cost an add AND, as a second value that
        // lives across the branch and the e0 / e1 ping-pong, a register copy at the end of the branch body.  The
        // boundary is read at gaddr + 8 (an immediate offset of the LDS read) and gaddr is stepped in place last.
        gst<double>(rec, (ws.gaddr << 6) + ws.rbase, fma(ws.gnext - ws.gd, cv, ws.kacc));
        kn = (gdn - ws.gnext) * cv;
        ws.gnext = lds_ld(ws.gaddr + 8u);
        ws.gaddr += 8u;
    }
    ws.kacc = kn;
    ws.gd = gdn;
    return cross;
}

// kOptExit: the rest of the list pass of merge_step, entries K0 .. NP-1, in chunks that end at compile-time boundaries.  A chunk
// over [K0, K1) writes t_k = min(max(x, s_k), s_{k+1}) for its entries, reading R[K1] as the pass found it (in place, in
// ascending k).  If no lane has x > R[K1] -- an ordered compare whose 64-bit result is the ballot, and a scalar branch --
// then t_k = s_k for every k >= K1 in every lane: the list is sorted, so x <= s_k <= s_{k+1}.  The pass stops there, exactly,
// ties included.  A sentinel x (the popped row is exhausted) is above every live key and runs to the end of the live
// prefix like any other.  The last chunk closes with t_{NP-1} = max(x, s_{NP-1}) as the full pass does.
// Every test is a scalar branch that the wave waits for, and a wave alone on its SIMD has nobody to hide it behind: with 64
// unrelated wavenumbers per wave two tests (4, 10) measured faster than three or four.  With the lanes grouped over rows
// (LaneRow) most steps leave at the first test, and three boundaries measured faster than 4/10, 3/9 and 2/5/9/14; with 64 rows
// of one wavenumber per wave the lanes re-enter shallower still, and 2/6/11 measured faster than 3/7/12 and 3/8
constexpr int kExitBounds[] = {2, 6, 11};
constexpr int kNoExitBound = 1000;
// the first boundary above k0
__host__ __device__ constexpr int merge_exit_bound(int k0)
{
    for (int b : kExitBounds)
        if (b > k0) return b;
    return kNoExitBound;
}
template <int K0, int NP, int NR>
__device__ __forceinline__ void merge_pass_exit(double (&R)[NR], double x)
{
    // the last boundary leaves at least two entries to the closing chunk
    constexpr int K1 = merge_exit_bound(K0) < NP - 2 ? merge_exit_bound(K0) : NP - 1;
    double mk[K1 - K0 > 0 ? K1 - K0 : 1];
#pragma unroll
    for (int k = K0; k < K1; ++k) asm("v_max_f64 %0, %1, %2" : "=v"(mk[k - K0]) : "v"(x), "v"(R[k]));
#pragma unroll
    for (int k = K0; k < K1; ++k) asm("v_min_f64 %0, %1, %2" : "=v"(R[k]) : "v"(mk[k - K0]), "v"(R[k + 1]));
    if constexpr (K1 == NP - 1) {
        asm("v_max_f64 %0, %1, %2" : "=v"(R[NP - 1]) : "v"(x), "v"(R[NP - 1]));
    } else {
        if (__builtin_amdgcn_ballot_w64(x > R[K1]) != 0) merge_pass_exit<K1, NP>(R, x);
    }
}

// The heads of the G rows are kept as a SORTED LIST IN REGISTERS (R[0] = the current winner): popping is free and the
// row's next key is inserted by one pass of v_max_f64 + v_min_f64 pairs over statically indexed
// registers -- no tree in LDS, no lane-dependent addressing, and the next winner is known after the FIRST
// compare-exchange, so its operands' LDS reads are hidden behind the rest of the pass and the walk.  NR = list length
// (compile time, >= G; unused entries hold "huge" keys).
// Returns the consumed element's (row, column) and whether it closed a bin, as 16 bits: the gradient kernel
// records them and replays the sorted order for the gradient rows.
template <int NR, bool W32, bool REC_CODE = false, bool SORTED = true, bool NODIV = false, int NP = NR, int OPT = 0>
__device__ __forceinline__ unsigned merge_step(double (&R)[NR], MergeElem &e, MergeElem &en, WalkState &ws,
                                               int lane, const double *A, const double *B,
                                               const double *DG, const double *GORD, double *rec,
                                               const unsigned char *PA = nullptr, const unsigned char *PB = nullptr,
                                               const MergeOrient &mo = MergeOrient{})
{
    static_assert(NP >= 1 && NP <= NR, "pass length");
    static_assert(OPT == 0 || (SORTED && NODIV && !REC_CODE), "the fast path");
    static_assert(merge_opt_valid(OPT), "OPT == 0 || (OPT & ~kOptTable) == (kOptBfi | kOptExit | kOptOrient)");
    // 1. the popped row's next element x enters the list s_1 <= s_2 <= ... (s_0 was popped):
    //        t_0 = min(x, s_1),   t_k = min(max(x, s_k), s_{k+1}),   t_{NP-1} = max(x, s_{NP-1})
    //    -- every output independent of the others (no carry chain), in place in ascending k.
    //    NP = pass length: the pass reads and writes R[0..NP) only, which is the full pass whenever R[NP..NR) hold nothing
    //    but "huge" keys (see the peeled steps of k_ck_overlap for when that is known without looking).
    const double x = OPT != 0 ? pack_key11_next(e.ai + e.bn, (unsigned)e.np, mo.inc) : pack_key11(e.ai + e.bn, e.ci, e.np);
    if constexpr (NP == 1) {
        R[0] = x;                               // the last element's step: its row's next key is a sentinel, nothing follows
    } else {
    asm("v_min_f64 %0, %1, %2" : "=v"(R[0]) : "v"(x), "v"(R[1]));
    // 2. fetch the operands of the new winner (LDS reads in flight during the rest of the pass and the walk)
    merge_fetch<W32, SORTED, OPT>(R[0], lane, A, B, DG, en, PA, PB, mo);
    if constexpr (OPT != 0) {
        merge_pass_exit<1, NP>(R, x);
    } else {
    // 3. finish the insertion: every max first, then every min -- no result is consumed by a neighbouring instruction
    //    (6.40 -> 6.32 ms against blocks of 6, same box)
    constexpr int kBlk = NP;
#pragma unroll
    for (int k0 = 1; k0 < NP - 1; k0 += kBlk) {
        double mk[kBlk];
#pragma unroll
        for (int j = 0; j < kBlk; ++j)
            if (k0 + j < NP - 1) asm("v_max_f64 %0, %1, %2" : "=v"(mk[j]) : "v"(x), "v"(R[k0 + j]));
#pragma unroll
        for (int j = 0; j < kBlk; ++j)
            if (k0 + j < NP - 1) asm("v_min_f64 %0, %1, %2" : "=v"(R[k0 + j]) : "v"(mk[j]), "v"(R[k0 + j + 1]));
    }
    asm("v_max_f64 %0, %1, %2" : "=v"(R[NP - 1]) : "v"(x), "v"(R[NP - 1]));
    }
    }
    // 4. rank walk on the element just consumed
    bool cross;
    if constexpr (NODIV) cross = merge_walk_nodiv(e, ws, rec);
    else cross = merge_walk<REC_CODE>(e, ws, rec, GORD, lane);
    // step code of the gradient replay, 12 bits: row (0-4), column (5-9), "the element closed a bin" (10); kCodesPerWord of
    // them to a 64-bit word of the stream
    return (unsigned)(e.ci | ((e.np - 1) << 5) | (cross ? 0x400 : 0));
}

// The last G - 1 steps of a merge, with the list pass shrinking by one entry per step.
//
// Every row has exactly one entry in the list: the key of its next element, or -- once its last element has been popped --
// the key formed from B[G] = "huge" (merge_fetch: an exhausted row re-enters as a sentinel, not as a live key).  The list is
// sorted and every sentinel is above every live key, so the live keys are a prefix of it.  When step t (0-based) begins,
// R[0] is element t itself and G*G - t elements are left including it; each live entry is the head of a different row with at
// least one of them, so at most min(G, G*G - t) entries are live and R[j] is a sentinel for every j >= G*G - t.  Step t pops
// R[0] and inserts x into R[1..): a pass over R[0 .. G*G - t) sees every live key, and what it leaves out it would have
// reproduced (min / max of sentinels among themselves -- which sentinel ends where may differ, none is ever consumed).
// The bound depends on t alone: no test, no ballot.  R[j] can first be dropped at step t = G*G - j, i.e. the steps
// t <= G*G - G need all G entries and step t = G*G - NP, NP = G-1 ... 1, needs NP of them.  (Entries G .. NR-1 of a launch with
// G < NR are sentinels from the start; the main loop still passes over them, its length being a template constant.)
// The bodies are instantiated for NP = NR-1 ... 1 and the first NR - G of them are skipped (G is wave-uniform).  Which of
// e0 / e1 holds the current element alternates per step; the caller hands it over in e1 when G and NR have the same parity
// and in e0 when not (swap_elems), so the choice is a compile-time one here.
template <int NP, int NR, bool W32, bool SORTED, bool NODIV, int OPT = 0>
__device__ __forceinline__ void merge_peel(double (&R)[NR], MergeElem &e0, MergeElem &e1, WalkState &ws, int G,
                                           int lane, const double *A, const double *B, const double *DG,
                                           const double *GORD, double *rec, const unsigned char *PA,
                                           const unsigned char *PB, const MergeOrient &mo = MergeOrient{})
{
    if constexpr (NP >= 1) {
        if (NP < G) {
            if constexpr (((NR - NP) & 1) != 0)
                merge_step<NR, W32, false, SORTED, NODIV, NP, OPT>(R, e1, e0, ws, lane, A, B, DG, GORD, rec, PA, PB, mo);
            else
                merge_step<NR, W32, false, SORTED, NODIV, NP, OPT>(R, e0, e1, ws, lane, A, B, DG, GORD, rec, PA, PB, mo);
        }
        merge_peel<NP - 1, NR, W32, SORTED, NODIV, OPT>(R, e0, e1, ws, G, lane, A, B, DG, GORD, rec, PA, PB, mo);
    }
}

// R[i] = head of row i = a_i + b_0: ascending in i when a is.  A loaded gas is (fast path: by precondition; generic: sorted
// first); a MERGED spectrum is non-decreasing only up to the rounding of its bin averages, and two neighbours that
// rounding has swapped can fall on either side of a key boundary (seen with k(g) flat to 1e-9: an unsorted list loses an
// entry in the insertion network and a sentinel is consumed).  So the keys are checked, and when some lane's are not
// ascending the heads are put in order one by one (the merge itself only needs every ROW ascending, i.e. b sorted).
// (the same check and reorder for the oriented heads below; merge_init keeps its own copy, so that the instantiations without
// kOptOrient are compiled from the text they always had)
template <int NR>
__device__ __forceinline__ void merge_init_order(double (&R)[NR], int G, double huge)
{
    bool bad = false;
#pragma unroll
    for (int i = 0; i + 1 < NR; ++i) bad |= (R[i + 1] < R[i]);
    if (__builtin_amdgcn_ballot_w64(bad) != 0) {
        double T[NR];
#pragma unroll
        for (int i = 0; i < NR; ++i) { T[i] = R[i]; R[i] = huge; }
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            if (i < G) {
                const double x = T[i];
#pragma unroll
                for (int k = NR - 1; k >= 1; --k) R[k] = fmin(fmax(x, R[k - 1]), R[k]);
                R[0] = fmin(x, R[0]);
            }
        }
    }
}
template <int NR>
__device__ __forceinline__ void merge_init(double (&R)[NR], int G, int lane, const double *A, double b0, double huge)
{
#pragma unroll
    for (int i = 0; i < NR; ++i) R[i] = (i < G) ? pack_key11(A[(i < G ? i : 0) * kWave + lane] + b0, i, 0) : huge;
    bool bad = false;
#pragma unroll
    for (int i = 0; i + 1 < NR; ++i) bad |= (R[i + 1] < R[i]);
    if (__builtin_amdgcn_ballot_w64(bad) != 0) {
        double T[NR];
#pragma unroll
        for (int i = 0; i < NR; ++i) { T[i] = R[i]; R[i] = huge; }
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            if (i < G) {
                const double x = T[i];
#pragma unroll
                for (int k = NR - 1; k >= 1; --k) R[k] = fmin(fmax(x, R[k - 1]), R[k]);
                R[0] = fmin(x, R[0]);
            }
        }
    }
}
// kOptOrient: the heads of this lane's rows, the row index at this lane's bit offset (column 0 in either packing)
template <int NR>
__device__ __forceinline__ void merge_init(double (&R)[NR], int G, const MergeOrient &mo, double huge)
{
    const double c0 = lds_ld(mo.cbase);
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const unsigned long long b = (unsigned long long)__double_as_longlong(lds_ld(mo.rbase + (unsigned)(i < G ? i : 0) * 512u) + c0);
        R[i] = (i < G) ? __longlong_as_double((long long)((b & ~0x7FFULL) | (unsigned long long)((unsigned)i << mo.rsh))) : huge;
    }
    merge_init_order<NR>(R, G, huge);
}

// ---- row-major merges (kOptRowMajor): the sorted order known before the first step --------------------------------------------
// With kOptOrient the rows are the operand with the larger top ordinate, and where the other operand is negligible beside it the
// G x G sums sort row by row: r_0 + c_0 .. r_0 + c_{G-1}, r_1 + c_0, ...  The list merge pops keys in ascending order, and within a
// row the keys ascend strictly (the sums are monotone in the column, and the column is in the low bits in both packings), so
// the popped order is row-major iff K(i, G-1) < K(i+1, 0) for every i + 1 < G -- the doubles the list itself compares, ties
// included.  R holds the heads K(i, 0) as merge_init left them: in a lane whose heads were not ascending they are the sorted
// heads instead, and such a lane fails by itself (passing would put K(i, 0) < K(i, G-1) < R[i+1] for every i, i.e. row i's
// head among the i + 1 smallest for every i, i.e. the heads ascending).  lane_passes: this lane's own verdict (the pattern
// bytes of the wavenumber order, merge_order_inverse).
//
// The partial form (merge_suffix_row): rows i0 .. G-1 are a separable SUFFIX when every key of the rows below i0 is below
// K(i0, 0) and the rows from i0 on sort row by row.  With M(i) = max over i' <= i of K(i', G-1), the largest key of the rows 0 .. i,
// that is M(i) < R[i+1] for every i in i0-1 .. G-2 -- boundary i of the test, with the running maximum in the place of K(i, G-1).
// (A merged operand ascends only up to rounding, so K(i', G-1) <= K(i, G-1) for i' < i is not given; where every boundary
// passes the K(i, G-1) ascend through the heads between them and M(i) = K(i, G-1): the full verdict is what it was.)
// It also covers a lane whose heads merge_init_order put in order: the rows 0 .. i have their heads below M(i) < R[i+1], so they
// are the i + 1 smallest heads, for every i >= i0-1 -- R[i] is row i's own head for every i >= i0 and R[0 .. i0) are the heads
// of the rows below i0, sorted.  The list merge of those rows then pops its G * i0 keys, all below R[i0], in the order the full
// merge does, the sentinels of its exhausted rows sink past R[i0 .. G), and what follows is rows i0 .. G-1 row by row.
// Returns the wave's i0: the upper row of the last boundary that some active lane fails, plus one -- 0 (every lane passes every
// boundary: the whole merge is walked), or 2 .. G (G: the boundary G-2 fails, no suffix; 1 does not occur).
template <int NR>
__device__ __forceinline__ int merge_rowmajor_test(const double (&R)[NR], int G, const MergeOrient &mo, bool &lane_passes)
{
    const double cl = lds_ld(mo.cbase + (unsigned)(G - 1) * 512u);
    const unsigned lowc = (unsigned)(G - 1) << mo.csh;
    bool fail = false;
    int i0 = 0;
    double top = 0.0;
#pragma unroll
    for (int i = 0; i + 1 < NR; ++i) {
        const unsigned long long b = (unsigned long long)__double_as_longlong(lds_ld(mo.rbase + (unsigned)(i < G ? i : 0) * 512u) + cl);
        const double last = __longlong_as_double((long long)((b & ~0x7FFULL) | (unsigned long long)(((unsigned)i << mo.rsh) | lowc)));
        if (i == 0) top = last;
        else asm("v_max_f64 %0, %1, %2" : "=v"(top) : "v"(top), "v"(last));
        const bool f = (i + 1 < G) & !(top < R[i + 1]);
        fail |= f;
        if (__builtin_amdgcn_ballot_w64(f) != 0) i0 = i + 2;       // the compare's own mask and scalar code
    }
    lane_passes = !fail;
    return i0;
}
// The test as the lists shorter than kSuffixMinList run it, which take a merge whole or not at all: K(i, G-1) < R[i+1] for every
// boundary, every active lane (the same verdict as i0 = 0 above; no running maximum, no row)
template <int NR>
__device__ __forceinline__ bool merge_rowmajor_whole(const double (&R)[NR], int G, const MergeOrient &mo, bool &lane_passes)
{
    const double cl = lds_ld(mo.cbase + (unsigned)(G - 1) * 512u);
    const unsigned lowc = (unsigned)(G - 1) << mo.csh;
    bool fail = false;
#pragma unroll
    for (int i = 0; i + 1 < NR; ++i) {
        const unsigned long long b = (unsigned long long)__double_as_longlong(lds_ld(mo.rbase + (unsigned)(i < G ? i : 0) * 512u) + cl);
        const double last = __longlong_as_double((long long)((b & ~0x7FFULL) | (unsigned long long)(((unsigned)i << mo.rsh) | lowc)));
        fail |= (i + 1 < G) & !(last < R[i + 1]);
    }
    lane_passes = !fail;
    return __builtin_amdgcn_ballot_w64(fail) == 0;
}
// The shortest suffix that is walked: below it the merge keeps the list to its end (measured)
constexpr int kSuffixMinRows = 1;
// The row from which a merge is walked, from the test's i0: 0 the whole merge, G none of it (the list with its peeled tail),
// between them G * i0 full-length list steps and then the rows i0 .. G-1
__device__ __forceinline__ int merge_suffix_row(int i0, int G, bool suffix_on)
{
    return i0 == 0 || (suffix_on && i0 <= G - kSuffixMinRows) ? i0 : G;
}
// The columns j < merge_rowmajor_sure_cols(NR) exist in every launch of list length NR: the launcher takes the smallest list
// length >= G (merge_list_len: 8, 10, 16, 20, 32) and the division-free walk needs G >= 2.  Saves the guard j < G, nothing else.
__host__ __device__ constexpr int merge_rowmajor_sure_cols(int NR)
{
    return NR == 10 ? 9 : NR == 16 ? 11 : NR == 20 ? 17 : NR == 32 ? 21 : 2;
}
// One row of a row-major merge: the walk over its G elements, the row's entry, the columns and the row of the (symmetric) weight
// table in registers
template <int NR>
__device__ __forceinline__ void merge_rowmajor_row(double ai, const double (&c)[NR], const double (&w)[NR], int G, WalkState &ws,
                                                   double *rec)
{
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        if (j < merge_rowmajor_sure_cols(NR) || j < G) {
            MergeElem e;
            e.ai = ai; e.bc = c[j]; e.w = w[j];
            merge_walk_nodiv(e, ws, rec);
        }
    }
}
template <int NR>
__device__ __forceinline__ void merge_rowmajor_weights(double (&w)[NR], double &ai, int i, int G, const MergeOrient &mo)
{
    // WT[(j << 5) | i]: one address for the whole wave, the column an immediate offset
    const unsigned wa = kLdsWT + ((unsigned)i << 3);
    ai = lds_ld(mo.rbase + ((unsigned)i << 9));
#pragma unroll
    for (int j = 0; j < NR; ++j) w[j] = lds_ld(wa + (unsigned)(j < merge_rowmajor_sure_cols(NR) || j < G ? j : 0) * 256u);
}
// The walk of the rows i0 .. G-1 of a merge whose test gave i0 (0: the whole merge; else ws comes from the list phase of the rows
// below), without the list: the same elements in the same order through the same merge_walk_nodiv, so ws ends as the list path leaves it.  Row and column are loop counters, the columns stay in registers
// (where the list kept its heads), and the weights and the entry of row i + 1 are read while row i is walked -- nothing
// depends on a value fetched in the step before.  Two rows per trip: the two sets of weights alternate without a copy.
template <int NR>
__device__ __forceinline__ void merge_rowmajor(int i0, int G, const MergeOrient &mo, WalkState &ws, double *rec)
{
    double c[NR], w0[NR], a0;
#pragma unroll
    for (int j = 0; j < NR; ++j) c[j] = lds_ld(mo.cbase + (unsigned)(j < G ? j : 0) * 512u);
    if constexpr (NR > 20) {
        // arrays of 32 weights beside the 32 columns do not fit the registers of two waves per SIMD: a weight is read for its step
        for (int i = i0; i < G; ++i) {
            const unsigned wa = kLdsWT + ((unsigned)i << 3);
            a0 = lds_ld(mo.rbase + ((unsigned)i << 9));
#pragma unroll
            for (int j = 0; j < NR; ++j) {
                if (j < merge_rowmajor_sure_cols(NR) || j < G) {
                    MergeElem e;
                    e.ai = a0; e.bc = c[j]; e.w = lds_ld(wa + (unsigned)j * 256u);
                    merge_walk_nodiv(e, ws, rec);
                }
            }
        }
        return;
    }
    double w1[NR], a1;
    merge_rowmajor_weights<NR>(w0, a0, i0, G, mo);
    for (int i = i0; i < G; i += 2) {
        merge_rowmajor_weights<NR>(w1, a1, i + 1 < G ? i + 1 : i, G, mo);
        merge_rowmajor_row<NR>(a0, c, w0, G, ws, rec);
        if (i + 1 < G) {
            merge_rowmajor_weights<NR>(w0, a0, i + 2 < G ? i + 2 : i, G, mo);
            merge_rowmajor_row<NR>(a1, c, w1, G, ws, rec);
        }
    }
}

// ---- whole walks on the launch's static schedule (kFlagStatic; MergeStatic in ansfm_merge_plan.h) --------------------------------
// A wave that walks a WHOLE merge (i0 == 0) starts at gd = 0 and adds WT[i][j] in row-major order in every lane: gd, the verdict
// gdn >= gnext of every element, the factors gnext - gd and gdn - gnext of a crossing and the bin it closes are the same in
// every lane, every merge and every tile of the launch.  merge_static_build forms them on the host by the recurrence of
// merge_walk_nodiv, and the block's prologue copies them into LDS behind the weight table (merge_static_fill).  The walk keeps
// what is per lane: cv = row + column and kacc = fma(cv, w, kacc), and at a crossing fma(C1, cv, kacc) and C2 * cv -- the
// operations of merge_walk_nodiv on the doubles it would have formed, so every closed sum has its bits.  No gd, no compare,
// no exec mask: whether an element closes a bin is a bit of the row's mask, tested by scalar code.
// The suffix form (0 < i0 < G) keeps merge_rowmajor: its gd comes out of a list phase whose order is per lane, so it is not
// uniform and no schedule applies.
// Closed bins stay on chip.  The schedule is valid only if bin b closes in row b or later; entry b of the rows operand has then
// been read (it is in a register before row b's first element), and A's slot b is free in either orientation: a lane whose
// rows are a is past it, a lane whose rows are b holds a as its columns, which are in registers from the start of the walk.
// So the closed sum goes to A[b] un-normalised (one LDS write, no record in global memory) and the kernel's end pass divides
// in place.  Nothing inside the walk reads scalar memory: the waits stay counted LDS waits.
constexpr unsigned kStaticRD = 0, kStaticC = kMaxG * 16u, kStaticMask = 2u * kMaxG * 16u;    // byte offsets in the static tables
static_assert(kStaticMask + kMaxG * 4u == kMergeStaticLds, "the plan's LDS arithmetic");
__device__ __forceinline__ unsigned merge_static_base(int G) { return kLdsWT + weight_table_bytes(G); }
typedef __attribute__((address_space(3))) dbl2 lds_dbl2;
typedef __attribute__((address_space(3))) unsigned lds_uint;
__device__ __forceinline__ dbl2 lds_ld2(unsigned a) { return *(const lds_dbl2 *)(size_t)a; }
// n / d from (r, d), r the refined reciprocal of d: fast_div's quotient and residual step on fast_div's own r (merge_static_fill)
__device__ __forceinline__ double recip_div(double n, dbl2 rd)
{
    const double q = n * rd.x;
    return fma(fma(-rd.y, q, n), rd.x, q);
}
// Prologue, lanes of wave 0: (reciprocal, width) of every bin -- v_rcp_f64 and fast_div's two Newton steps, on the device because
// the hardware reciprocal is not the host's -- and the schedule from the kernel arguments
__device__ __forceinline__ void merge_static_fill(const OverlapParams &p, int G, int lane)
{
    const unsigned sb = merge_static_base(G);
    if (lane < G) {
        const double d = p.g_ord[lane + 1] - p.g_ord[lane];
        double r = __builtin_amdgcn_rcp(d);
        r = fma(fma(-d, r, 1.0), r, r);
        r = fma(fma(-d, r, 1.0), r, r);
        *(lds_dbl2 *)(size_t)(sb + kStaticRD + (unsigned)lane * 16u) = dbl2{r, d};
    }
    if (lane < kMaxG) {
        *(lds_dbl2 *)(size_t)(sb + kStaticC + (unsigned)lane * 16u) = dbl2{p.st.c1[lane], p.st.c2[lane]};
        *(lds_uint *)(size_t)(sb + kStaticMask + (unsigned)lane * 4u) = p.st.rowmask[lane];
    }
}
struct StaticWalk {
    double kacc;
    dbl2 cc;            // (C1, C2) of the next crossing, read when the one before it closed
    unsigned caddr;     // its LDS address; entry 32 of a G = 32 schedule is read and never used (the masks follow)
    unsigned oaddr;     // this lane's slot of A for the bin that closes next
};
template <bool TEST>
__device__ __forceinline__ void merge_static_elem(int j, double cv, double w, unsigned mask, StaticWalk &sw)
{
    if (TEST && ((mask >> j) & 1u) != 0) {
        lds_st(sw.oaddr, fma(sw.cc.x, cv, sw.kacc));
        sw.kacc = sw.cc.y * cv;
        sw.oaddr += 512u;
        sw.caddr += 16u;
        sw.cc = lds_ld2(sw.caddr);
    } else
        sw.kacc = fma(cv, w, sw.kacc);
}
// One row.  With the Gauss-Legendre weights a row's crossings sit at its first or last column (bin b closes where row b ends,
// up to rounding), so the columns that every launch of the list length has, the first aside, run straight through unless the mask
// names one of them; the first and the columns from merge_rowmajor_sure_cols on test their bit.  Lists above 20 read a weight
// for its step (merge_rowmajor), w is unused there.
template <int NR>
__device__ __forceinline__ void merge_static_row(double ai, const double (&c)[NR], const double (&w)[NR], unsigned wa, unsigned mask,
                                                 int G, StaticWalk &sw)
{
    constexpr int kSure = merge_rowmajor_sure_cols(NR);
    constexpr unsigned kInner = ((1u << kSure) - 1u) & ~1u;
    const auto weight = [&](int j) { if constexpr (NR > 20) return lds_ld(wa + (unsigned)j * 256u); else return w[j]; };
    merge_static_elem<true>(0, ai + c[0], weight(0), mask, sw);
    if ((mask & kInner) == 0) {
#pragma unroll
        for (int j = 1; j < kSure; ++j) merge_static_elem<false>(j, ai + c[j], weight(j), mask, sw);
    } else {
#pragma unroll
        for (int j = 1; j < kSure; ++j) merge_static_elem<true>(j, ai + c[j], weight(j), mask, sw);
    }
#pragma unroll
    for (int j = kSure; j < NR; ++j)
        if (j < G) merge_static_elem<true>(j, ai + c[j], weight(j), mask, sw);
}
__device__ __forceinline__ unsigned merge_static_mask(unsigned sb, int i)
{
    return *(const lds_uint *)(size_t)(sb + kStaticMask + ((unsigned)i << 2));
}
// The whole walk; returns kacc of the open bin.  a_lane: the LDS address of this lane's entry of A's row 0.  The rows are read
// as merge_rowmajor reads them, a row ahead, and the row's mask with them (one v_readfirstlane when its row begins).
template <int NR>
__device__ __forceinline__ double merge_rowmajor_static(int G, const MergeOrient &mo, unsigned a_lane)
{
    const unsigned sb = merge_static_base(G);
    double c[NR], w0[NR], a0;
#pragma unroll
    for (int j = 0; j < NR; ++j) c[j] = lds_ld(mo.cbase + (unsigned)(j < G ? j : 0) * 512u);
    StaticWalk sw;
    sw.kacc = 0.0;
    sw.caddr = sb + kStaticC;
    sw.cc = lds_ld2(sw.caddr);
    sw.oaddr = a_lane;
    if constexpr (NR > 20) {
        for (int i = 0; i < G; ++i) {
            a0 = lds_ld(mo.rbase + ((unsigned)i << 9));
            const unsigned m = (unsigned)__builtin_amdgcn_readfirstlane((int)merge_static_mask(sb, i));
            merge_static_row<NR>(a0, c, c, kLdsWT + ((unsigned)i << 3), m, G, sw);
        }
        return sw.kacc;
    }
    double w1[NR], a1;
    unsigned m0 = merge_static_mask(sb, 0), m1;
    merge_rowmajor_weights<NR>(w0, a0, 0, G, mo);
    for (int i = 0; i < G; i += 2) {
        const int i1 = i + 1 < G ? i + 1 : i;
        m1 = merge_static_mask(sb, i1);
        merge_rowmajor_weights<NR>(w1, a1, i1, G, mo);
        merge_static_row<NR>(a0, c, w0, 0u, (unsigned)__builtin_amdgcn_readfirstlane((int)m0), G, sw);
        if (i + 1 < G) {
            const int i2 = i + 2 < G ? i + 2 : i;
            m0 = merge_static_mask(sb, i2);
            merge_rowmajor_weights<NR>(w0, a0, i2, G, mo);
            merge_static_row<NR>(a1, c, w1, 0u, (unsigned)__builtin_amdgcn_readfirstlane((int)m1), G, sw);
        }
    }
    return sw.kacc;
}

// Per-lane insertion sort of one LDS column (values ascending, stable) carrying the original index of every
// position in P.  Only the generic path (k not sorted in g) uses it.
__device__ __forceinline__ void sort_column(double *X, unsigned char *P, int G, int lane)
{
    for (int g = 0; g < G; ++g) P[g * kWave + lane] = (unsigned char)g;
    for (int i = 1; i < G; ++i) {
        const double key = X[i * kWave + lane];
        const unsigned char pk = P[i * kWave + lane];
        int j = i - 1;
        while (j >= 0 && X[j * kWave + lane] > key) {
            X[(j + 1) * kWave + lane] = X[j * kWave + lane];
            P[(j + 1) * kWave + lane] = P[j * kWave + lane];
            --j;
        }
        X[(j + 1) * kWave + lane] = key;
        P[(j + 1) * kWave + lane] = pk;
    }
}

}  // namespace ansfm

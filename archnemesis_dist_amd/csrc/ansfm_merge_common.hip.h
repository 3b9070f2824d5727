// ansfm_merge_common.hip.h -- device-side pieces shared by the merge kernels' translation units (ansfm_api.hip,
// ansfm_merge32.hip): the ln-k table encoding and (P,T) interpolation of calc_k (Spectroscopy_0.py:2298-2437), the
// parameter block, the table reads of one gas, LDS / global access helpers and the per-XCD tile queues.  Templates
// and inline device functions only -- no kernels -- so that it can be included from more than one translation unit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ansfm_merge_plan.h"       // kWave, kMaxG, kLaneNV and the other constants the launch plan shares with the kernels

namespace ansfm {

// ------------------------------------------------------------------------------------------------
// ln-k table encoding.  k > 0  -> ln k (finite double)
//                       k <= 0 -> quiet NaN whose 51 payload bits are the top 51 bits of k
// (sign, exponent, 39 mantissa bits: exact for tables that were float32 on disk).  The
// good/bad/mixed corner logic of calc_k (Spectroscopy_0.py:2391-2403) needs the sign and, for the
// all-non-positive "bad" branch, the raw value.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double encode_lnk(double k)
{
    if (k > 0.0) return log(k);
    unsigned long long b = (unsigned long long)__double_as_longlong(k);
    unsigned long long box = 0x7FF8000000000000ULL | (b >> 13);
    return __longlong_as_double((long long)box);
}
__device__ __forceinline__ bool lnk_is_boxed(double x) { return x != x; }
__device__ __forceinline__ double lnk_unbox(double x)
{
    unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return __longlong_as_double((long long)((b & 0x0007FFFFFFFFFFFFULL) << 13));
}

// Per (model, layer) interpolation constants: the nearest-then-bracket corner choice of calc_k
// (Spectroscopy_0.py:2336-2389) is wave-uniform, so it is computed once per layer.
struct LayerInterp {
    int ipl, iph, itl, ith;
    double v, u, dudt;
};


// The bilinear form in ln k of the merge kernels' table reads, (1-v)(1-u) l1 + v(1-u) h1 + v u h2 + (1-v) u l2, with the
// multiply-adds written out: left to the compiler's contraction, the sum of four products came out in different orders in
// interp_k and in interp_k_nobox (which product is the plain multiply), i.e. with different last bits.  The order is the
// one the compiler had chosen for interp_k.
__device__ __forceinline__ double interp_lnk(double l1, double l2, double h1, double h2, double v, double u)
{
    return fma((1.0 - v) * u, l2, fma(v * u, h2, fma((1.0 - v) * (1.0 - u), l1, (v * (1.0 - u)) * h1)));
}

// k for one (corner set, u, v): Spectroscopy_0.py:2391-2403 (+ dk/dT :2241-2247 when wanted)
__device__ __forceinline__ double interp_k(double l1, double l2, double h1, double h2, double v,
                                           double u)
{
    // l1 = (ip_low,it_low)  l2 = (ip_low,it_high)  h1 = (ip_high,it_low)  h2 = (ip_high,it_high)
    bool b1 = lnk_is_boxed(l1), b2 = lnk_is_boxed(l2), b3 = lnk_is_boxed(h1), b4 = lnk_is_boxed(h2);
    double kk = 0.0;
    if (!(b1 | b2 | b3 | b4)) {
        const double x = interp_lnk(l1, l2, h1, h2, v, u);
        kk = exp(x);
    } else if (b1 & b2 & b3 & b4) {
        double klo1 = lnk_unbox(l1), klo2 = lnk_unbox(l2), khi1 = lnk_unbox(h1), khi2 = lnk_unbox(h2);
        kk = (1.0 - v) * (1.0 - u) * klo1 + v * (1.0 - u) * khi1 + v * u * khi2 + (1.0 - v) * u * klo2;
    }
    return kk;
}
// interp_k for a table without a boxed entry (OverlapParams / ansfm_ktable_has_boxed: none of its W * G * NP * NT * S values
// is <= 0 or NaN): only the first branch of interp_k can be taken, so the four tests, their reduction and the two exec-mask
// regions go -- interp_lnk and exp() are interp_k's, the result is the same double.  The pad lanes of the last
// wavenumber tile (w >= W) still hold the boxed 0 the relayout kernels write there: x and exp(x) are NaN in them and one
// v_max_f64 against 0 returns the 0 that interp_k gives (the instruction returns its other operand for a NaN; exp() of a
// real entry is > 0 or +0 and passes unchanged).
__device__ __forceinline__ double interp_k_nobox(double l1, double l2, double h1, double h2, double v, double u)
{
    const double ex = exp(interp_lnk(l1, l2, h1, h2, v, u));
    double kk;
    asm("v_max_f64 %0, %1, 0" : "=v"(kk) : "v"(ex));
    return kk;
}
__device__ __forceinline__ void interp_kg(double l1, double l2, double h1, double h2, double v,
                                          double u, double dudt, double &kk, double &dk)
{
    bool b1 = lnk_is_boxed(l1), b2 = lnk_is_boxed(l2), b3 = lnk_is_boxed(h1), b4 = lnk_is_boxed(h2);
    kk = 0.0; dk = 0.0;
    if (!(b1 | b2 | b3 | b4)) {
        double x = (1.0 - v) * (1.0 - u) * l1 + v * (1.0 - u) * h1 + v * u * h2 + (1.0 - v) * u * l2;
        kk = exp(x);
        double dxdt = (-l1 * (1.0 - v) - h1 * v + h2 * v + l2 * (1.0 - v)) * dudt;
        dk = kk * dxdt;
    } else if (b1 & b2 & b3 & b4) {
        double klo1 = lnk_unbox(l1), klo2 = lnk_unbox(l2), khi1 = lnk_unbox(h1), khi2 = lnk_unbox(h2);
        kk = (1.0 - v) * (1.0 - u) * klo1 + v * (1.0 - u) * khi1 + v * u * khi2 + (1.0 - v) * u * klo2;
        dk = (-klo1 * (1.0 - v) - khi1 * v + khi2 * v + klo2 * (1.0 - v)) * dudt;
    }
}


struct OverlapParams {
    const double *lnK;        // [NP][NT][S][G][Wpad]            (FROM_K: unused)
    const double *kin;        // FROM_K: k[S][L][G][Wpad] (array-level k_overlap seam)
    const LayerInterp *li;    // [n][L]
    const double *amount;     // [n][S][L]
    const double *del_g;      // [G]
    double *tau;              // [n][L][G][Wpad]
    double *scratch;          // [gridDim.x][2][G][64]
    int *err_flag;            // bit0: unsorted input k-distribution
    unsigned int *tile_counter;  // [8] dynamic tile queues, one per XCD (zeroed before every launch)
    int W, Wpad, G, NT, S, L, n_models;
    int delg_f32;             // DELG is a float32 array: del_g[i]*del_g[j] is a float32 product
    double g_ord[kMaxG + 2];  // [0, cumsum(del_g)] (float32 cumsum when delg_f32), g_ord[G]=1, NaN
    const double *lnKg;       // [NP][NT][S][Wpad][Gs], Gs = gfast_stride(G): the g-fastest copy of lnK, or null (load_gas_rows)
    // [Wpad] each, or both null: a wavenumber's walk pattern of the launch before and of this one (merge_order_inverse);
    // two buffers, so that no wave reads a byte that a wave of the same launch wrote
    const unsigned char *hint_in;
    unsigned char *hint_out;
    // the static schedule of a whole row-major walk (merge_static_build); read only by a launch with kFlagStatic, which copies
    // it into LDS in its prologue
    MergeStatic st;
};
// The g-fastest copy of the table (k_table_gfast builds it from lnK): the G ordinates of one (p, T, gas, wavenumber) lie as one
// run of Gs doubles, G rounded up to even so that every run starts 16-byte aligned and is read as Gs / 2 pairs; the pad
// ordinate of an odd G holds the boxed 0 and is never consumed.
__host__ __device__ constexpr int gfast_stride(int G) { return (G + 1) & ~1; }
typedef double lnk_pair __attribute__((ext_vector_type(2)));


// Table reads of one gas for one (64-wavenumber, layer) tile.  The loads of kLoadBatch g-ordinates (4 corner
// rows each) are all issued before the first value is used: one memory round trip per batch instead of one per
// g-ordinate (a wave has at most one sibling on its SIMD to hide it behind).  Indices are clamped, not
// predicated, so the batch stays branch-free.
constexpr int kLoadBatch = 10;

// NONNEG (the 32-bit-key merge kernel, ansfm_merge32.hip.h): a negative value counts as "unsorted" too (that kernel
// orders float32 bit patterns as unsigned integers) and -0.0 is stored as +0.0.
// NOBOX: the table holds no boxed entry (interp_k_nobox).
template <bool FROM_K, bool NONNEG = false, bool NOBOX = false>
__device__ __forceinline__ void load_gas(const OverlapParams &p, const LayerInterp &q, int m, int l,
                                         int s, int nu, double *DST, int lane, bool &unsorted)
{
    const int G = p.G;
    const double amt = p.amount[((size_t)m * p.S + s) * p.L + l];
    double prev = NONNEG ? 0.0 : -__builtin_inf();
    if constexpr (FROM_K) {
        const double *src = p.kin + (((size_t)s * p.L + l) * G) * p.Wpad + nu;
        for (int g0 = 0; g0 < G; g0 += kLoadBatch) {
            double r[kLoadBatch];
#pragma unroll
            for (int k = 0; k < kLoadBatch; ++k) {
                const int gi = (g0 + k < G) ? g0 + k : G - 1;
                r[k] = src[(size_t)gi * p.Wpad];
            }
#pragma unroll
            for (int k = 0; k < kLoadBatch; ++k)
                if (g0 + k < G) {
                    double kk = r[k] * amt;
                    if constexpr (NONNEG) kk += 0.0;
                    DST[(g0 + k) * kWave + lane] = kk;
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
                // streamed once per tile: non-temporal so the table does not push the merge scratch out of L2
                r1[k] = __builtin_nontemporal_load(c1 + go);
                r2[k] = __builtin_nontemporal_load(c2 + go);
                r3[k] = __builtin_nontemporal_load(c3 + go);
                r4[k] = __builtin_nontemporal_load(c4 + go);
            }
#pragma unroll
            for (int k = 0; k < kLoadBatch; ++k)
                if (g0 + k < G) {
                    double kk = (NOBOX ? interp_k_nobox(r1[k], r2[k], r3[k], r4[k], q.v, q.u)
                                       : interp_k(r1[k], r2[k], r3[k], r4[k], q.v, q.u)) * amt;
                    if constexpr (NONNEG) kk += 0.0;
                    DST[(g0 + k) * kWave + lane] = kk;
                    unsorted |= (kk < prev);
                    prev = kk;
                }
        }
    }
}

// Layer-grouped lanes (the forward kernel's fast path).  The (model, layer) rows of a launch are one row axis of
// length R = n_models * L, and the cells of a 64-wavenumber block are numbered (wavenumber / width, row, wavenumber % width),
// the last fastest; a tile is 64 consecutive cells of that order: width wavenumbers x 64 / width consecutive rows, running on
// into the next wavenumber group at the end of the row axis (width: 1 or kLaneNV, see below).  A block holds 64 * R cells,
// i.e. exactly R tiles, whatever R is.
// Neighbouring rows of one wavenumber meet the same gases at nearby (p, T), so the lanes of a wave re-enter the head list at
// similar depths and merge_pass_exit can stop where a wave of 64 unrelated wavenumbers cannot.  What was wave-uniform in the
// other mapping -- the row's interpolation constants, its amounts, the corner rows of the table -- is per lane here.
static_assert(kLaneNV == 2 || kLaneNV == 4 || kLaneNV == 8, "group width");
// The width a launch runs at is wave-uniform run-time data, 1 or kLaneNV ("pairs"), an argument of k_ck_overlap beside flags: the
// functions below take its binary logarithm, nvs.  At width 1 a tile is 64 consecutive rows of ONE wavenumber, running on into
// the next wavenumber at the end of the row axis: whether a merge sorts row by row (merge_rowmajor_test) and how deep a lane
// re-enters the head list are decided by the gases' magnitudes at the wavenumber, so a second wavenumber in the wave is an
// independent draw that spoils the first.
constexpr unsigned kLaneNVShift = (unsigned)__builtin_ctz((unsigned)kLaneNV);

// Queue order inside a 64-wavenumber block: the u-th tile handed out is tile lane_tile_of(u) of the cell order.  A tile is at
// "row slot" s when it is the s-th tile that starts in its wavenumber group; the tiles go out slot by slot, group by group
// within a slot, so that the 16 / width tiles that read the same 128-byte table lines (one 16-wavenumber span, one row
// slot) are neighbours in the queue and one wave's miss serves the others from L2.  Every group has R / Q such tiles or
// one more (Q = 64 / width, the rows of a tile and the groups of a block); the i-th group that has one more is group
// i * Q / (R % Q).
__host__ __device__ constexpr unsigned lane_tile_of(unsigned u, unsigned R, unsigned nvs)
{
    const unsigned qs = 6u - nvs, Q = 1u << qs;
    const unsigned fl = R >> qs, rem = R & (Q - 1u);
    unsigned grp = u & (Q - 1u), slot = u >> qs;
    if (u >= (fl << qs)) { slot = fl; grp = ((u - (fl << qs)) << qs) / rem; }
    return ((grp * R + Q - 1u) >> qs) + slot;       // the first tile that starts in the group, + slot
}

// Cell c of a block's cell order (c = tile * 64 + lane): its wavenumber inside the block and its row
struct LaneCell { unsigned w, row; };
__host__ __device__ constexpr LaneCell lane_cell(unsigned c, unsigned R, unsigned nvs)
{
    const unsigned pair = c >> nvs;                 // width 1: pair = c, grp = c / R, w = grp
    const unsigned grp = pair / R;
    return LaneCell{(grp << nvs) + (c & ((1u << nvs) - 1u)), pair - grp * R};
}

// The two functions above, checked where they are compiled: at each width the queue order is a permutation of the block's R
// tiles and the cells of tile k are distinct cells of the 64 x R block (a bijection, since there are 64 * R of them) ...
__host__ __device__ constexpr bool lane_mapping_holds(unsigned R, unsigned nvs)
{
    for (unsigned k = 0; k < R; ++k) {
        unsigned hits = 0;
        for (unsigned u = 0; u < R; ++u) hits += lane_tile_of(u, R, nvs) == k ? 1u : 0u;
        if (hits != 1u) return false;
    }
    for (unsigned c = 0; c < 64u * R; ++c) {
        const LaneCell x = lane_cell(c, R, nvs);
        if (x.w >= 64u || x.row >= R) return false;
        if ((((x.w >> nvs) * R + x.row) << nvs) + (x.w & ((1u << nvs) - 1u)) != c) return false;     // the inverse
    }
    return true;
}
static_assert(lane_mapping_holds(1, 0) && lane_mapping_holds(3, 0) && lane_mapping_holds(33, 0) && lane_mapping_holds(64, 0) &&
              lane_mapping_holds(100, 0), "width 1");
static_assert(lane_mapping_holds(1, kLaneNVShift) && lane_mapping_holds(3, kLaneNVShift) && lane_mapping_holds(33, kLaneNVShift) &&
              lane_mapping_holds(64, kLaneNVShift) && lane_mapping_holds(100, kLaneNVShift), "width kLaneNV");
// ... and at these spots they give what the plain-Python model of the mapping gives (tests/test_merge_one_wavenumber_model.py
// reads the two tables and compares them with tests/test_merge_layer_groups_model.py).  {u, R, width, tile} and
// {tile, lane, R, width, wavenumber in the block, row}
constexpr unsigned kLaneTileSpots[][4] = {
    {0, 100, 1, 0}, {1, 100, 1, 2}, {37, 100, 1, 58}, {50, 100, 1, 79}, {64, 100, 1, 1}, {98, 100, 1, 95}, {99, 100, 1, 98},
    {0, 100, 2, 0}, {1, 100, 2, 4}, {37, 100, 2, 17}, {50, 100, 2, 58}, {64, 100, 2, 2}, {98, 100, 2, 53}, {99, 100, 2, 78},
    {1, 33, 1, 1}, {16, 33, 1, 16}, {32, 33, 1, 32}, {1, 33, 2, 2}, {16, 33, 2, 17}, {31, 33, 2, 32}, {32, 33, 2, 1},
    {2, 3, 1, 2}, {1, 696, 1, 11}, {37, 696, 1, 403}, {64, 696, 1, 1}, {348, 696, 1, 310}, {694, 696, 1, 674}, {695, 696, 1, 685}};
constexpr unsigned kLaneCellSpots[][6] = {
    {0, 0, 100, 1, 0, 0}, {1, 36, 100, 1, 1, 0}, {99, 63, 100, 1, 63, 99}, {50, 17, 100, 1, 32, 17},
    {0, 0, 100, 2, 0, 0}, {1, 36, 100, 2, 0, 50}, {99, 63, 100, 2, 63, 99}, {50, 17, 100, 2, 33, 8},
    {1, 36, 33, 1, 3, 1}, {32, 63, 33, 1, 63, 32}, {16, 17, 33, 1, 31, 18}, {1, 36, 3, 2, 32, 2}, {2, 63, 3, 2, 63, 2}, {1, 17, 3, 2, 27, 1}};
__host__ __device__ constexpr bool lane_spots_hold()
{
    for (const auto &t : kLaneTileSpots)
        if ((t[2] != 1u && t[2] != (unsigned)kLaneNV) || lane_tile_of(t[0], t[1], t[2] == 1u ? 0u : kLaneNVShift) != t[3]) return false;
    for (const auto &t : kLaneCellSpots) {
        if (t[3] != 1u && t[3] != (unsigned)kLaneNV) return false;
        const LaneCell x = lane_cell(t[0] * 64u + t[1], t[2], t[3] == 1u ? 0u : kLaneNVShift);
        if (x.w != t[4] || x.row != t[5]) return false;
    }
    return true;
}
static_assert(lane_spots_hold(), "lane_tile_of / lane_cell against the model's values");

// The order of a block's wavenumbers (width 1, the launches of MergePlan::order).  Whether a merge sorts row by row is a
// property of the wavenumber, and a tile of R % 64 != 0 runs on into the next wavenumber: the 64 wavenumbers of a block are
// handed out sorted by the pattern byte the launch before wrote for them (k_ck_overlap: the verdicts of merge_rowmajor_test
// for merges 1 .. 8 at row R / 2, merge 1 in the most significant bit), so that a tile that straddles mostly joins like with like.
// Lane i of the wave holds the byte of wavenumber i of the block, 0xFF for a pad wavenumber (they stay behind the real ones);
// the key (byte << 6) | i keeps equal bytes in wavenumber order, so all-zero bytes give the identity.  A wavenumber's position
// is its rank, the number of smaller keys; lane_cell's group index is a position, and the wavenumber at position q is the
// inverse permutation at q.  Which cell a lane holds changes nothing in what is computed for the cell.
__host__ __device__ constexpr unsigned merge_order_key(unsigned byte, unsigned i) { return (byte << 6) | i; }
// the rank of wavenumber i among the 64 bytes b(0) .. b(63): what merge_order_inverse counts lane by lane
template <class F>
__host__ __device__ constexpr unsigned merge_order_rank(F &&b, unsigned i)
{
    unsigned r = 0;
    for (unsigned j = 0; j < 64u; ++j) r += merge_order_key(b(j), j) < merge_order_key(b(i), i) ? 1u : 0u;
    return r;
}
// ... held to the values of the plain-Python model (tests/test_merge_order_model.py reads the table and the formula's constants):
// the bytes b(i) = (i * 37 + 11) & 0xE0 for i < 58 and 0xFF behind them, {wavenumber of the block, its position}
constexpr unsigned kOrderSpotReal = 58, kOrderSpotMul = 37, kOrderSpotAdd = 11, kOrderSpotMask = 0xE0;
__host__ __device__ constexpr unsigned merge_order_spot_byte(unsigned i)
{
    return i < kOrderSpotReal ? (i * kOrderSpotMul + kOrderSpotAdd) & kOrderSpotMask : 0xFFu;
}
constexpr unsigned kOrderSpots[][2] = {{0, 0}, {1, 7}, {2, 15}, {3, 22}, {6, 50}, {7, 1}, {13, 51}, {31, 31}, {57, 21}, {58, 58}, {63, 63}};
__host__ __device__ constexpr bool order_spots_hold()
{
    for (const auto &t : kOrderSpots)
        if (merge_order_rank([](unsigned i) { return merge_order_spot_byte(i); }, t[0]) != t[1]) return false;
    for (unsigned i = 0; i < 64u; ++i)                  // all-zero bytes: the identity
        if (merge_order_rank([](unsigned) { return 0u; }, i) != i) return false;
    return true;
}
static_assert(order_spots_hold(), "merge_order_rank against the model's values");

// inv, per lane: the wavenumber (of block vt) at position `lane`.  The 64 bytes are read once per tile; every lane is active.
// nonzero: the lane's wavenumber is a real one and its byte is not 0 (ansfm_last_merge_order counts them).
__device__ __forceinline__ int merge_order_inverse(const unsigned char *hint_in, int vt, int W, int lane, bool &nonzero)
{
    const int nu = vt * kWave + lane;
    const unsigned byte = nu < W ? (unsigned)hint_in[nu] : 0xFFu;
    nonzero = nu < W && byte != 0u;
    const unsigned key = merge_order_key(byte, (unsigned)lane);
    unsigned rank = 0;
#pragma unroll
    for (int j = 0; j < kWave; ++j) rank += (unsigned)__builtin_amdgcn_readlane((int)key, j) < key ? 1u : 0u;
    // lane i sends i to lane rank(i): the ranks are a permutation of the lanes, every lane receives one value
    return __builtin_amdgcn_ds_permute((int)(rank << 2), lane);
}

struct LaneRow {
    int nu;                     // wavenumber of the lane's cell; W <= nu < Wpad: a pad cell
    unsigned row;               // m * L + l: the row of li and of tau
    unsigned arow, krow;        // index of gas 0's amount, (m * S) * L + l, and (FROM_K) the layer l
    size_t o1, o2, o3, o4;      // the four corner rows of load_gas as element offsets into lnK, + nu; with the g-fastest
                                // copy: the lane's runs of gas 0 as element offsets into lnKg
    double v, u;
};
// the cell of lane `lane` of tile k of wavenumber block vt; gfast: the launch reads the g-fastest copy (wave-uniform);
// ordered (wave-uniform, width 1): the cell's wavenumber index is a position in the block's order, inv = merge_order_inverse
template <bool FROM_K>
__device__ __forceinline__ LaneRow lane_row(const OverlapParams &p, int vt, unsigned k, int lane, unsigned nvs, bool gfast,
                                            bool ordered = false, int inv = 0)
{
    const unsigned R = (unsigned)p.n_models * (unsigned)p.L;
    const LaneCell cell = lane_cell(k * kWave + (unsigned)lane, R, nvs);
    LaneRow lr;
    lr.row = cell.row;
    lr.nu = vt * kWave + (ordered ? __builtin_amdgcn_ds_bpermute((int)(cell.w << 2), inv) : (int)cell.w);
    const unsigned m = lr.row / (unsigned)p.L;
    lr.krow = lr.row - m * (unsigned)p.L;
    lr.arow = m * (unsigned)p.S * (unsigned)p.L + lr.krow;
    lr.o1 = lr.o2 = lr.o3 = lr.o4 = 0;
    lr.v = lr.u = 0.0;
    if constexpr (!FROM_K) {
        const LayerInterp q = p.li[lr.row];
        // a (p, T) block holds S * G * Wpad doubles in lnK and S * Wpad * Gs in lnKg, where wavenumber nu starts at nu * Gs
        const size_t strideT = (size_t)p.S * (gfast ? gfast_stride(p.G) : p.G) * p.Wpad;
        const size_t own = gfast ? (size_t)lr.nu * gfast_stride(p.G) : (size_t)lr.nu;
        lr.o1 = ((size_t)q.ipl * p.NT + q.itl) * strideT + own;
        lr.o2 = ((size_t)q.ipl * p.NT + q.ith) * strideT + own;
        lr.o3 = ((size_t)q.iph * p.NT + q.itl) * strideT + own;
        lr.o4 = ((size_t)q.iph * p.NT + q.ith) * strideT + own;
        lr.v = q.v; lr.u = q.u;
    }
    return lr;
}

// load_gas for layer-grouped lanes: the same reads, the same interp_k / interp_k_nobox and the same `* amt` per cell, with
// the row a per-lane value.  gfast (wave-uniform, lr from lane_row with the same value): the table branch reads the g-fastest
// copy, a lane's ordinates of one corner as consecutive 16-byte pairs of its own run; the same doubles reach the same r1 .. r4.
// GFAST is a parameter of this function, not of the kernel: the caller branches on the launch's flag around two whole copies of
// loads + interpolation.  One copy with the branch around the loads alone joins the two kinds of loads in front of the first
// use, where every load has to have landed: the wave-fastest reads measured 0.08 ms slower at C2 that way.
template <bool FROM_K, bool NOBOX, bool GFAST>
__device__ __forceinline__ void load_gas_rows(const OverlapParams &p, const LaneRow &lr, int s, double *DST, int lane,
                                              bool &unsorted)
{
    constexpr bool gfast = GFAST && !FROM_K;
    const int G = p.G;
    const double amt = p.amount[(size_t)lr.arow + (size_t)s * p.L];
    double prev = -__builtin_inf();
    if constexpr (FROM_K) {
        const double *src = p.kin + (((size_t)s * p.L + lr.krow) * G) * p.Wpad + lr.nu;
        for (int g0 = 0; g0 < G; g0 += kLoadBatch) {
            double r[kLoadBatch];
#pragma unroll
            for (int k = 0; k < kLoadBatch; ++k) {
                const int gi = (g0 + k < G) ? g0 + k : G - 1;
                r[k] = src[(size_t)gi * p.Wpad];
            }
#pragma unroll
            for (int k = 0; k < kLoadBatch; ++k)
                if (g0 + k < G) {
                    const double kk = r[k] * amt;
                    DST[(g0 + k) * kWave + lane] = kk;
                    unsorted |= (kk < prev);
                    prev = kk;
                }
        }
    } else {
        static_assert(kLoadBatch % 2 == 0, "a batch is whole pairs of ordinates");
        const int Gs = gfast_stride(G);
        const double *base = gfast ? p.lnKg + (size_t)s * p.Wpad * Gs : p.lnK + (size_t)s * G * p.Wpad;
        const double *c1 = base + lr.o1, *c2 = base + lr.o2, *c3 = base + lr.o3, *c4 = base + lr.o4;
        for (int g0 = 0; g0 < G; g0 += kLoadBatch) {
            double r1[kLoadBatch], r2[kLoadBatch], r3[kLoadBatch], r4[kLoadBatch];
            if constexpr (gfast) {
#pragma unroll
                for (int k = 0; k < kLoadBatch; k += 2) {
                    // the pair (g0 + k, g0 + k + 1); past the end the last pair, (Gs - 2, Gs - 1), as the last ordinate below
                    const int gi = (g0 + k < Gs) ? g0 + k : Gs - 2;
                    const lnk_pair x1 = *reinterpret_cast<const lnk_pair *>(c1 + gi);
                    const lnk_pair x2 = *reinterpret_cast<const lnk_pair *>(c2 + gi);
                    const lnk_pair x3 = *reinterpret_cast<const lnk_pair *>(c3 + gi);
                    const lnk_pair x4 = *reinterpret_cast<const lnk_pair *>(c4 + gi);
                    r1[k] = x1.x; r1[k + 1] = x1.y;
                    r2[k] = x2.x; r2[k + 1] = x2.y;
                    r3[k] = x3.x; r3[k + 1] = x3.y;
                    r4[k] = x4.x; r4[k + 1] = x4.y;
                }
            } else {
#pragma unroll
                for (int k = 0; k < kLoadBatch; ++k) {
                    const int gi = (g0 + k < G) ? g0 + k : G - 1;
                    const size_t go = (size_t)gi * p.Wpad;
                    // plain loads, not load_gas's non-temporal ones: a 128-byte table line serves the 16 / width tiles of its
                    // 16-wavenumber span, which the queue hands out together (measured at C2: 4.27 -> 4.13 ms at width 2; at width 1,
                    // where a line serves 16 tiles in 8-byte pieces, 3.97 ms non-temporal against 3.55 plain)
                    r1[k] = c1[go];
                    r2[k] = c2[go];
                    r3[k] = c3[go];
                    r4[k] = c4[go];
                }
            }
#pragma unroll
            for (int k = 0; k < kLoadBatch; ++k)
                if (g0 + k < G) {
                    const double kk = (NOBOX ? interp_k_nobox(r1[k], r2[k], r3[k], r4[k], lr.v, lr.u)
                                             : interp_k(r1[k], r2[k], r3[k], r4[k], lr.v, lr.u)) * amt;
                    DST[(g0 + k) * kWave + lane] = kk;
                    unsorted |= (kk < prev);
                    prev = kk;
                }
        }
    }
}

__device__ __forceinline__ double fast_div(double n, double d)
{   // n/d with v_rcp_f64 + 2 Newton steps + residual correction (<= ~1 ulp; frac of rank()).  One Newton step gives the
    // same quotients (tools/calib/div_check.hip) but k_ck_overlap measured 1.2 % SLOWER with it (5.88 -> 5.95 ms, same box,
    // twice): the second step's two instructions fill issue slots the resolve otherwise leaves empty
    double r = __builtin_amdgcn_rcp(d);
    r = fma(fma(-d, r, 1.0), r, r);
    r = fma(fma(-d, r, 1.0), r, r);
    double q = n * r;
    return fma(fma(-d, q, n), r, q);
}


typedef __attribute__((address_space(3))) double lds_double;
__device__ __forceinline__ unsigned lds_addr(const double *p) { return (unsigned)(size_t)(const lds_double *)p; }
__device__ __forceinline__ double lds_ld(unsigned a) { return *(const lds_double *)(size_t)a; }
__device__ __forceinline__ void lds_st(unsigned a, double v) { *(lds_double *)(size_t)a = v; }
// Global access as wave-uniform base + 32-bit byte offset: the compiler emits `global_load/store v_off, s[base]` and the
// per-access address arithmetic stays 32-bit (64-bit pointer adds are multi-pass VALU instructions).
template <class T> __device__ __forceinline__ T gld(const void *base, unsigned byte_off)
{
    return *reinterpret_cast<const T *>(reinterpret_cast<const char *>(base) + byte_off);
}
template <class T> __device__ __forceinline__ void gst(void *base, unsigned byte_off, T v)
{
    *reinterpret_cast<T *>(reinterpret_cast<char *>(base) + byte_off) = v;
}

typedef __attribute__((address_space(3))) float lds_float;
__device__ __forceinline__ float lds_ldf(unsigned a) { return *(const lds_float *)(size_t)a; }

// Dynamic tile queues.  With 5 resident waves per CU one SIMD hosts two waves that run slower than the solo
// ones; static striding would make the launch wait for them.  One relaxed atomic per tile (~2800*7 merge steps
// of work) -- every wave exits when the counters pass the tile counts.
// Eight queues, queue q = wavenumber tiles vt with vt % 8 == q (layer fastest): the layers of one wavenumber
// tile share k-table corner rows, so they are kept on one XCD's L2.  A wave starts on the queue of the XCD it
// runs on (HW_REG_XCC_ID; affinity only, any placement is correct) and steals from the others when its own
// is empty.
struct TileQueue {
    int myq, qoff;
    __device__ __forceinline__ void init()
    {
        myq = (int)(__builtin_amdgcn_s_getreg((20) | (0 << 6) | ((4 - 1) << 11)) & 7);
        qoff = 0;
    }
    __device__ __forceinline__ bool next(const OverlapParams &p, int lane, int &vt, int &m, int &l)
    {
        const int NVT = p.Wpad / kWave;
        while (qoff < 8) {
            const int qq = (myq + qoff) & 7;
            const int nvt_q = (NVT - qq + 7) / 8;                     // tiles vt = qq, qq+8, ...
            const long nq = (long)p.n_models * nvt_q * p.L;
            unsigned int tq = 0;
            if (lane == 0 && nq > 0) tq = atomicAdd(p.tile_counter + qq, 1u);
            const long t = (long)__builtin_amdgcn_readfirstlane(tq);
            if (nq > 0 && t < nq) {
                l = (int)(t % p.L);
                const long r = t / p.L;
                vt = qq + 8 * (int)(r % nvt_q);
                m = (int)(r / nvt_q);
                return true;
            }
            ++qoff;
        }
        return false;
    }
    // Layer-grouped lanes: the same eight queues over the 64-wavenumber blocks, so a block's table rows stay on one XCD; a
    // block's R = n_models * L tiles go out in the order of lane_tile_of at the launch's width.  k = the tile's index in the block's cell order.
    __device__ __forceinline__ bool next_rows(const OverlapParams &p, int lane, unsigned nvs, int &vt, unsigned &k)
    {
        const int NVT = p.Wpad / kWave;
        const unsigned R = (unsigned)p.n_models * (unsigned)p.L;
        while (qoff < 8) {
            const int qq = (myq + qoff) & 7;
            const int nvt_q = (NVT - qq + 7) / 8;
            const long nq = (long)nvt_q * R;
            unsigned int tq = 0;
            if (lane == 0 && nq > 0) tq = atomicAdd(p.tile_counter + qq, 1u);
            const long t = (long)__builtin_amdgcn_readfirstlane(tq);
            if (nq > 0 && t < nq) {
                const unsigned b = (unsigned)(t / R);
                vt = qq + 8 * (int)b;
                k = lane_tile_of((unsigned)t - b * R, R, nvs);
                return true;
            }
            ++qoff;
        }
        return false;
    }
};


}  // namespace ansfm

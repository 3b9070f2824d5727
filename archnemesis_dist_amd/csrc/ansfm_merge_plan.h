// ansfm_merge_plan.h -- how a forward merge is launched, decided on the host from integers alone: the constants the merge
// kernels and their launchers share, the switches of the environment (MergeSwitches), the facts of one call (MergeCall) and
// the plan that follows from the two (merge_plan -> MergePlan: which k_ck_overlap, its block, LDS, grid and arguments, and
// what ansfm_last_merge_* report), and the static schedule of a whole row-major walk, formed from the call's weights
// (merge_g_ord, merge_static_build -> MergeStatic; tests/host/merge_static_main.cpp).  No HIP header: a plain C++17 compiler builds it (tests/host/merge_plan_main.cpp); the
// kernel headers include it for the constants.  DESIGN.md 4.1, "The launch plan".
#pragma once
#include <float.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#if defined(__HIPCC__)
#define ANSFM_HD __host__ __device__
#else
#define ANSFM_HD
#endif

namespace ansfm {

constexpr int kWave = 64;
constexpr int kMaxG = 32;

// The bits of OPT as ansfm_last_merge_launch reports them.  Value 4 (a late read of the bin boundary, retired) stays unused.
constexpr int kOptTable = 1, kOptBfi = 2, kOptExit = 8, kOptOrient = 16;
constexpr int kMergeOpt = kOptTable | kOptBfi | kOptExit | kOptOrient;
// reported beside them, a launch parameter and not a bit of OPT: the lanes of a wave are grouped over rows (k_ck_overlap's argument lane_rows)
constexpr int kOptLaneRows = 32;
// likewise a launch parameter (bit 1 of the same argument, instantiations with kOptTable only): a wave whose lanes' merges all
// sort row by row walks them without the head list (merge_rowmajor)
constexpr int kOptRowMajor = 64;
constexpr int kFlagLaneRows = 1, kFlagRowMajor = 2;      // k_ck_overlap's argument flags
// a further bit of flags, set only with kFlagLaneRows and a table launch, reported by ansfm_last_merge_table_layout and not in the
// trims: the table is read from its g-fastest copy (OverlapParams::lnKg, load_gas_rows)
constexpr int kFlagTableGfast = 4;
// a further bit, never set by default and read by the table kernels only: ANSFM_MERGE_SUFFIX=0, a merge that is not row-major
// from its first row keeps the head list to its end (merge_suffix_row)
constexpr int kFlagSuffixOff = 8;
// two further bits, read by the table kernels of the lists from kStaticMinList entries only and not in the trims: the launch
// carries a valid static schedule of the whole walk (MergeStatic; its tables and the reciprocals of the bin widths follow the
// weight table in LDS), and ANSFM_MERGE_STATIC=0, a whole walk keeps the per-lane step (merge_rowmajor) all the same
constexpr int kFlagStatic = 16, kFlagStaticOff = 32;
// The only values instantiated: key repack, early exit and orientation travel together, the table is on top of them
ANSFM_HD constexpr bool merge_opt_valid(int opt) { return opt == 0 || (opt & ~kOptTable) == (kOptBfi | kOptExit | kOptOrient); }
// Rows of doubles per wave: a[G], b[G] and the sentinel column b[G]; with kOptOrient also a[G] = "huge", the sentinel column of a
// lane whose columns are a.  One block's waves still fit the CU's LDS as before at every instantiated list length.
ANSFM_HD constexpr int merge_wave_rows(int G, int opt) { return 2 * G + ((opt & kOptOrient) != 0 ? 2 : 1); }
// The product table WT[(col << 5) | row] with col <= G (an exhausted row's sentinel key names column G; its entry is read and
// never used), so (G + 1) * 32 doubles, shared by the waves of a block (at most kMaxBlockWaves)
constexpr int kMaxBlockWaves = 8;
ANSFM_HD constexpr unsigned weight_table_bytes(int G) { return (unsigned)(G + 1) * 32u * 8u; }
// the wavenumbers of a row-mapped tile with ANSFM_MERGE_LANES=pairs (ansfm_merge_common.hip.h, "Layer-grouped lanes")
constexpr int kLaneNV = 2;

constexpr size_t kCuLdsBytes = (size_t)160 * 1024;      // LDS of one CU (MI355X)
constexpr size_t kLdsGranule = 128;                     // measured (tools/calib/lds_granule.hip): 7 blocks up to 23 360 bytes
// the tables that open the 64-bit-key merge kernels' LDS block: del_g [kMaxG], g_ord [kMaxG + 2], the float32 copy of del_g
constexpr size_t kMergeLdsTables = (size_t)(2 * kMaxG + 2) * sizeof(double) + kMaxG * sizeof(float);

// length of the register-resident row-head list of the merge kernels: smallest instantiated size >= G
inline int merge_list_len(int G)
{
    static const int sizes[] = {8, 10, 16, 20, 32};
    for (int v : sizes) if (v >= G) return v;
    return 32;
}
// the shortest list at which a launch orders a block's wavenumbers (MergePlan::order)
constexpr int kMergeOrderMinList = 16;
// the shortest list whose kernels carry the walk of a list merge's separable top rows (MergePlan::suffix; a compile-time choice of
// k_ck_overlap by its list length, no bit of flags): measured at C2, G = 10 loses with every kSuffixMinRows (+0.02 ms of 0.98)
constexpr int kSuffixMinList = 16;
// the shortest list whose kernels carry the static schedule of a whole walk and the reciprocal table (MergePlan::static_tables;
// a compile-time choice as kSuffixMinList is: at G = 10 every fixed cost per merge has lost so far)
constexpr int kStaticMinList = 16;
// LDS of the static tables behind the weight table: (reciprocal, width) of every bin, the two factors of every crossing, and
// the crossing columns of every row as a bit mask
constexpr size_t kMergeStaticLds = (size_t)kMaxG * 16 + (size_t)kMaxG * 16 + (size_t)kMaxG * 4;

// g_ord = [0, cumsum(del_g)], g_ord[ng] = 1 (ForwardModel_0.py:6141-6143); float32 cumsum when DELG is.  G + 2 entries
inline void merge_g_ord(const double *del_g, int G, bool delg_f32, double *g_ord)
{
    double acc = 0.0;
    float accf = 0.0f;
    g_ord[0] = 0.0;
    for (int g = 0; g < G; ++g) {
        if (delg_f32) { accf += (float)del_g[g]; g_ord[g + 1] = (double)accf; }
        else { acc += del_g[g]; g_ord[g + 1] = acc; }
    }
    g_ord[G] = 1.0;
    g_ord[G + 1] = __builtin_nan("");           // never crossed: merge_walk compares with an ordered >=
}

// ---- the static schedule of a whole row-major walk (merge_rowmajor_static) ---------------------------------------------------
// A wave that walks a whole merge row by row meets the weights WT[i][j] in row-major order whatever its lanes hold (WT is
// symmetric, so neither does the lanes' orientation matter): the cumulative weight gd of merge_walk_nodiv, the verdict
// gdn >= gnext of every element, the two factors of a crossing and the bin it closes are functions of del_g and g_ord alone.
// They are formed here, once per launch, by the walk's own recurrence in the walk's own operations (IEEE adds, subtractions and
// ordered compares of doubles; the one multiplication is the float32 product the kernel's WT prologue forms), so the kernel
// takes them as constants and the sums it forms are the ones merge_walk_nodiv forms, bit for bit.
struct MergeStatic {
    unsigned rowmask[kMaxG];        // bit j of rowmask[i]: element (i, j) closes a bin
    double c1[kMaxG], c2[kMaxG];    // crossing n, in walk order, closes bin n: gnext - gd and gdn - gnext
    double gd_end, last_width;      // the final gd, and gd - g_ord[G - 1]: the divisor of the open last bin
    int nbins;                      // bins closed
    int valid;                      // the schedule may replace the walk
};
// g_ord: G + 2 entries as merge_params forms them, g_ord[G + 1] = NaN.  Valid means: every float32 factor and product is zero or
// a normal number (what the host and the device round alike whatever their denormal modes), and bin b closes in row b or later --
// then row b's entry of the rows operand has been read when the closed sum takes its slot.  The arrays are
// filled either way; NaN weights cross nothing (the compare is ordered) and leave the schedule invalid.
inline void merge_static_build(const double *del_g, const double *g_ord, int G, MergeStatic &s)
{
    memset(&s, 0, sizeof s);
    if (G < 2 || G > kMaxG) return;
    const auto plain = [](float v) { const float m = v < 0.0f ? -v : v; return v == 0.0f || (m >= FLT_MIN && m <= FLT_MAX); };
    bool ok = true;
    double gd = 0.0;
    int ig = 0;
    for (int i = 0; i < G; ++i) {
        for (int j = 0; j < G; ++j) {
            const float fi = (float)del_g[i], fj = (float)del_g[j];
            const float wf = fi * fj;
            ok = ok && plain(fi) && plain(fj) && plain(wf);
            const double w = (double)wf;
            const double gdn = gd + w;
            // an element closes at most one bin; ordered: g_ord[G + 1] is NaN (the guard keeps a caller's table without it in range)
            if (ig < G && gdn >= g_ord[ig + 1]) {
                ok = ok && ig <= i;
                s.rowmask[i] |= 1u << j;
                s.c1[ig] = g_ord[ig + 1] - gd;
                s.c2[ig] = gdn - g_ord[ig + 1];
                ++ig;
            }
            gd = gdn;
        }
    }
    s.nbins = ig;
    s.gd_end = gd;
    s.last_width = gd - g_ord[G - 1];
    s.valid = ok ? 1 : 0;
}
// f(std::integral_constant<int, D>) at D = merge_list_len(G): how a launcher names the instantiation for a run-time G
template <class F>
auto by_list_len(int G, F &&f)
{
    switch (merge_list_len(G)) {
        case 8: return f(std::integral_constant<int, 8>{});
        case 10: return f(std::integral_constant<int, 10>{});
        case 16: return f(std::integral_constant<int, 16>{});
        case 20: return f(std::integral_constant<int, 20>{});
        default: return f(std::integral_constant<int, 32>{});
    }
}

// grid of a merge launch: blocks per CU = 160 KiB / block_bytes within [1, max_per_cu], no more blocks than tiles, at least one
inline long merge_grid(int num_cus, size_t block_bytes, int max_per_cu, long ntiles)
{
    int per_cu = (int)(kCuLdsBytes / block_bytes);
    if (per_cu < 1) per_cu = 1;
    if (per_cu > max_per_cu) per_cu = max_per_cu;
    long grid = (long)num_cus * per_cu;
    if (grid > ntiles) grid = ntiles;
    return grid < 1 ? 1 : grid;
}

// The environment's overrides of the forward merge launch; every default means "not set"
struct MergeSwitches {
    enum Lanes { kLanesUnset, kLanesWavenumbers, kLanesPairs };
    bool walk_records = false;      // ANSFM_MERGE_WALK=records: the recorded walk, no division-free path
    bool load_boxtests = false;     // ANSFM_LOAD_BOXTESTS=1: keep the box tests of the table reads
    bool legacy = false;            // ANSFM_MERGE_LEGACY=1: the plain form of the division-free path (OPT = 0)
    int keys = 0;                   // ANSFM_MERGE_KEYS: 32 or, for any other value, 64; replaces ansfm_set_merge_keys' choice
    int waves_per_cu = 0;           // ANSFM_WAVES_PER_CU: honoured within [1, 8)
    Lanes lanes = kLanesUnset;      // ANSFM_MERGE_LANES=wavenumbers | pairs
    bool rowmajor_off = false;      // ANSFM_MERGE_ROWMAJOR=0
    bool layout_wave = false;       // ANSFM_TABLE_LAYOUT=wave: read lnK although a g-fastest copy exists
    bool order_off = false;         // ANSFM_MERGE_ORDER=0: a block's wavenumbers in their own order, no pattern bytes written
    bool suffix_off = false;        // ANSFM_MERGE_SUFFIX=0: no walk of the separable top rows behind a list phase
    bool static_off = false;        // ANSFM_MERGE_STATIC=0: a whole walk steps per lane although the launch has a static schedule
};
// read per launch: a caller may change the environment between two calls
inline MergeSwitches merge_switches_from_env()
{
    MergeSwitches sw;
    const auto is = [](const char *name, const char *value) { const char *ev = getenv(name); return ev && !strcmp(ev, value); };
    const auto starts = [](const char *name, char c) { const char *ev = getenv(name); return ev && ev[0] == c; };
    sw.walk_records = is("ANSFM_MERGE_WALK", "records");
    sw.load_boxtests = starts("ANSFM_LOAD_BOXTESTS", '1');
    sw.legacy = starts("ANSFM_MERGE_LEGACY", '1');
    if (const char *ev = getenv("ANSFM_MERGE_KEYS")) sw.keys = atoi(ev) == 32 ? 32 : 64;
    if (const char *ev = getenv("ANSFM_WAVES_PER_CU")) sw.waves_per_cu = atoi(ev);
    if (is("ANSFM_MERGE_LANES", "wavenumbers")) sw.lanes = MergeSwitches::kLanesWavenumbers;
    else if (is("ANSFM_MERGE_LANES", "pairs")) sw.lanes = MergeSwitches::kLanesPairs;
    sw.rowmajor_off = starts("ANSFM_MERGE_ROWMAJOR", '0');
    sw.layout_wave = is("ANSFM_TABLE_LAYOUT", "wave");
    sw.order_off = starts("ANSFM_MERGE_ORDER", '0');
    sw.suffix_off = starts("ANSFM_MERGE_SUFFIX", '0');
    sw.static_off = starts("ANSFM_MERGE_STATIC", '0');
    return sw;
}

// What the plan of one forward merge depends on
struct MergeCall {
    bool from_k = false;        // the array-level seam's k instead of the table
    bool generic = false;       // per-lane sort first, on request (the rerun of an unsorted call)
    bool monotone = false;      // the table's k(g) were found non-decreasing at upload
    bool has_boxed = true;      // the table holds an entry <= 0 or NaN
    bool delg_f32 = false;      // float32 weights
    int merge_keys = 64;        // ansfm_set_merge_keys
    int G = 0, S = 0, W = 0, Wpad = 0, L = 0, n_models = 0, num_cus = 0;
    // w00 = del_g[0]^2 in the weights' precision and g_ord[1]: the first merged element must not close a bin (rank()'s python
    // [-1] wrap, which only the recorded walk reproduces)
    double w00 = 0.0, g_ord1 = 0.0;
    // the g-fastest copy of the context's table (build_table_gfast): whether it exists, and the table's shape, which the call's must equal
    bool gfast_copy = false;
    int table_W = 0, table_Wpad = 0, table_G = 0, table_S = 0;
    size_t lds32 = 0;           // dynamic LDS of k_ck_overlap32 at this G and weight type (overlap32_lds_bytes)
    bool static_valid = false;  // merge_static_build found a valid schedule for the call's del_g
};

struct MergePlan {
    // the kernel: <NR = merge_list_len(G), FROM_K, W32 = delg_f32, SORTED = sorted, NODIV = nodiv, NOBOX = nobox, OPT = opt>,
    // or k_ck_overlap32 with keys32
    bool sorted = false, nodiv = false, nobox = false, keys32 = false;
    int opt = 0;
    // its arguments: flags (kFlag*) and the width of a row-mapped tile (1 or kLaneNV; 0 for OPT = 0, which does not read it)
    bool lane_rows = false, rowmajor = false, gfast = false;
    // a list merge walks its separable top rows (part of the walk: off with it, and with ANSFM_MERGE_SUFFIX=0, kFlagSuffixOff)
    bool suffix = false;
    // the block holds the static tables (kMergeStaticLds: a valid schedule, a table kernel of a list from kStaticMinList entries) and
    // normalises by the reciprocal table; and its whole walks run on the schedule (off with the walk and with ANSFM_MERGE_STATIC=0)
    bool static_tables = false, static_walk = false;
    int lane_nv = 0, flags = 0;
    // the launch hands a block's wavenumbers out in the order of their last walk patterns and writes this launch's patterns
    // (OverlapParams::hint_in / hint_out, which the launcher sets for such a plan only; no bit of flags or trims)
    bool order = false;
    // its launch: waves per block, dynamic LDS, blocks, and the bytes of ctx->scratch one block needs
    int nwaves = 1;
    size_t lds = 0;
    long grid = 1;
    size_t scratch_bytes_per_block = 0;
    // what ansfm_last_merge_launch and ansfm_last_merge_group_width report (the table layout is gfast, the waves nwaves)
    int trims = 0, group_width = 0;
};

// Every decision once, each from the call, the switches and the decisions above it
inline MergePlan merge_plan(const MergeCall &c, const MergeSwitches &sw)
{
    MergePlan m;
    // fast path: every k(g) non-decreasing (checked at upload for tables, in the kernel otherwise); generic path: per-lane
    // sort of each gas first
    m.sorted = !c.generic && (c.from_k || c.monotone);
    // The division-free walk (merge_walk_nodiv) and the 32-bit-key kernel need sorted, non-negative input and a first element
    // of the merged order that does not close a bin.  A negative value raises the same flag as an unsorted one in the 32-bit
    // kernel and the call is rerun on the generic path.
    m.nodiv = m.sorted && c.G >= 2 && c.w00 < c.g_ord1 && !sw.walk_records;
    // a table without a boxed entry is read without the box tests
    m.nobox = m.nodiv && !c.from_k && !c.has_boxed && !sw.load_boxtests;
    m.keys32 = m.nodiv && (sw.keys != 0 ? sw.keys : c.merge_keys) == 32;
    // the division-free path in its trimmed form.  The weight table is for float32 weights: the compiler contracts the walk's
    // gd + DG[i] * DG[j] with float64 weights into one fma, which no table of rounded products reproduces bit for bit (the
    // float32 product is rounded before it is widened, so its table is exact)
    const bool trimmed = m.nodiv && !sw.legacy && !m.keys32;
    m.opt = !trimmed ? 0 : c.delg_f32 ? kMergeOpt : (kMergeOpt & ~kOptTable);
    const bool table = (m.opt & kOptTable) != 0;

    // waves per CU: 8 at most, as one-wave blocks or as the waves of one block (the kernel's launch bound), fewer on request
    const int max_per_cu = sw.waves_per_cu >= 1 && sw.waves_per_cu < kMaxBlockWaves ? sw.waves_per_cu : kMaxBlockWaves;
    const size_t wave_bytes = (size_t)merge_wave_rows(c.G, m.opt) * kWave * sizeof(double);
    const long ntiles = (long)c.n_models * (c.Wpad / kWave) * c.L;
    if (table) {
        // one block per CU: the tables once, then as many waves' rows as the CU's 160 KiB hold (7 at G = 20); no more blocks
        // than the tiles need
        m.static_tables = c.static_valid && merge_list_len(c.G) >= kStaticMinList;
        const size_t shared_bytes = kMergeLdsTables + weight_table_bytes(c.G) + (m.static_tables ? kMergeStaticLds : 0);
        const int fit = (int)((kCuLdsBytes - shared_bytes) / wave_bytes);
        m.nwaves = fit < max_per_cu ? fit : max_per_cu;
        m.lds = shared_bytes + (size_t)m.nwaves * wave_bytes;
        const long per_cu = merge_grid(c.num_cus, m.lds, 1, ntiles), needed = (ntiles + m.nwaves - 1) / m.nwaves;
        m.grid = per_cu < needed ? per_cu : needed;
    } else {
        // one-wave blocks, per CU as many as fit by the LDS size rounded up to the granule
        m.nwaves = 1;
        m.lds = m.keys32 ? c.lds32 : wave_bytes + kMergeLdsTables + (m.sorted ? 0 : (size_t)2 * c.G * kWave);
        m.grid = merge_grid(c.num_cus, (m.lds + kLdsGranule - 1) / kLdsGranule * kLdsGranule, max_per_cu, ntiles);
    }
    m.scratch_bytes_per_block = (size_t)m.nwaves * 6 * c.G * kWave * sizeof(double);

    // the trimmed path groups a wave's lanes over rows (LaneRow: the same tiles per 64-wavenumber block, so the grid and the
    // queues hold).  64 wavenumbers of one row per wave remain for ANSFM_MERGE_LANES=wavenumbers and for a launch of 2^24 rows
    // or more, whose cell numbers would leave the 32 bits lane_row computes in
    m.lane_rows = m.opt != 0 && (long)c.n_models * c.L < (1L << 24) && sw.lanes != MergeSwitches::kLanesWavenumbers;
    // the width of a row-mapped tile: 1 wavenumber x 64 rows for every shape, or kLaneNV x 64 / kLaneNV with ANSFM_MERGE_LANES=pairs
    m.lane_nv = m.opt == 0 ? 0 : sw.lanes == MergeSwitches::kLanesPairs ? kLaneNV : 1;
    // the kernels with the weight table walk a wave's row-major merges without the head list, in either lane mapping
    m.rowmajor = table && !sw.rowmajor_off;
    // a row-mapped launch on the context's own table reads the g-fastest copy where the upload built one
    m.gfast = m.lane_rows && !c.from_k && c.gfast_copy && c.W == c.table_W && c.Wpad == c.table_Wpad && c.G == c.table_G &&
              c.S == c.table_S && !sw.layout_wave;
    // the walk's kernel at width 1 orders a block's wavenumbers by the pattern bytes of the launch before (merge_order_inverse)
    // where a list step is dear enough to pay for the ranking and the scattered table runs of every tile: list lengths from 16
    // (measured at C2: G = 16 -2.3 %, G = 20 -3.0 %, but G = 10 +1.4 % with the order against the same kernel without it)
    m.order = m.rowmajor && m.lane_rows && m.lane_nv == 1 && merge_list_len(c.G) >= kMergeOrderMinList && !sw.order_off;
    m.suffix = m.rowmajor && !sw.suffix_off && merge_list_len(c.G) >= kSuffixMinList;
    m.static_walk = m.static_tables && m.rowmajor && !sw.static_off;
    m.flags = (m.lane_rows ? kFlagLaneRows : 0) | (m.rowmajor ? kFlagRowMajor : 0) | (m.gfast ? kFlagTableGfast : 0) |
              (m.rowmajor && sw.suffix_off ? kFlagSuffixOff : 0) | (m.static_tables ? kFlagStatic : 0) |
              (m.static_tables && !m.static_walk ? kFlagStaticOff : 0);
    m.trims = m.opt | (m.lane_rows ? kOptLaneRows : 0) | (m.rowmajor ? kOptRowMajor : 0);
    m.group_width = m.lane_rows ? m.lane_nv : 0;
    return m;
}

}  // namespace ansfm

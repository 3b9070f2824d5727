// ansfm_overlap.hip -- translation unit of k_ck_overlap (ansfm_overlap_kernels.hip.h): the instantiations of the forward merge,
// their launcher, and the launch set-up it shares with the gradient merge (ansfm_overlapg.hip).
#include "ansfm_overlap_kernels.hip.h"
#include "ansfm_merge32_launch.h"
#include "ansfm_ctx.hip.h"

namespace ansfm {

void merge_params(ansfm_ctx *ctx, OverlapParams &p, const double *kin, int W, int Wpad, int G, int S, int L, int n_models,
                  const LayerInterp *li, const double *amount, const double *del_g_dev, const double *del_g_host, double *tau)
{
    p.lnK = ctx->lnK.as<double>();
    p.kin = kin;
    p.li = li;
    p.amount = amount;
    p.del_g = del_g_dev;
    p.tau = tau;
    p.err_flag = ctx->d_flag.as<int>() + 1;
    // eight tile queues, then the forward merge's two 64-bit totals (ansfm_last_merge_rowmajor): cleared by one memset
    p.tile_counter = reinterpret_cast<unsigned int *>(ctx->d_flag.as<int>() + kFlagTileCounter);
    p.W = W; p.Wpad = Wpad; p.G = G; p.NT = ctx->NT; p.S = S; p.L = L; p.n_models = n_models;
    p.delg_f32 = ctx->delg_f32;
    // g_ord = [0, cumsum(del_g)], g_ord[ng] = 1 (ForwardModel_0.py:6141-6143); float32 cumsum when DELG is
    double acc = 0.0;
    float accf = 0.0f;
    p.g_ord[0] = 0.0;
    for (int g = 0; g < G; ++g) {
        if (ctx->delg_f32) { accf += (float)del_g_host[g]; p.g_ord[g + 1] = (double)accf; }
        else { acc += del_g_host[g]; p.g_ord[g + 1] = acc; }
    }
    p.g_ord[G] = 1.0;
    p.g_ord[G + 1] = __builtin_nan("");        // never crossed: merge_walk compares with an ordered >=
}

constexpr size_t kCuLdsBytes = (size_t)160 * 1024;      // LDS of one CU (MI355X)

int merge_launch_begin(ansfm_ctx *ctx, const OverlapParams &p, size_t block_bytes, int max_per_cu,
                       std::initializer_list<MergeWorkspace> workspaces, long *grid_out)
{
    int per_cu = (int)(kCuLdsBytes / block_bytes);
    if (per_cu < 1) per_cu = 1;
    if (per_cu > max_per_cu) per_cu = max_per_cu;
    const long ntiles = (long)p.n_models * (p.Wpad / kWave) * p.L;
    long grid = (long)ctx->num_cus * per_cu;
    if (grid > ntiles) grid = ntiles;
    if (grid < 1) grid = 1;
    for (const MergeWorkspace &w : workspaces) HIPCHK(w.buf->reserve((size_t)grid * w.bytes_per_block));
    HIPCHK(hipMemsetAsync(p.tile_counter, 0, (8 + 4) * sizeof(unsigned int), ctx->stream));
    *grid_out = grid;
    return ANSFM_OK;
}

// the trims an instantiation of the fast path carries: the weight table only with float32 weights (see launch_overlap)
static constexpr int merge_opt_of(bool w32) { return w32 ? kMergeOpt : (kMergeOpt & ~kOptTable); }

int launch_overlap(ansfm_ctx *ctx, bool from_k, const double *kin, int W, int Wpad, int G, int S,
                   int L, int n_models, const LayerInterp *li, const double *amount,
                   const double *del_g_dev, const double *del_g_host, double *tau, bool generic)
{
    // fast path: every k(g) non-decreasing (checked at upload for tables, in the kernel otherwise); generic path:
    // per-lane sort of each gas first (k_ck_overlap<..., SORTED = false>), also on request (the rerun of an unsorted call)
    const bool sorted = !generic && (from_k || ctx->monotone);
    OverlapParams p;
    memset(&p, 0, sizeof p);
    merge_params(ctx, p, kin, W, Wpad, G, S, L, n_models, li, amount, del_g_dev, del_g_host, tau);
    // The division-free walk (merge_walk_nodiv) and the 32-bit-key kernel (ansfm_merge32.hip.h, opt-in) need sorted,
    // non-negative input and a first element of the merged order that does not close a bin (rank()'s python [-1] wrap,
    // which only the recorded walk reproduces).  A negative value raises the same flag as an unsorted one in the 32-bit
    // kernel and the call is rerun on the generic path.
    bool nodiv = sorted && G >= 2;
    if (nodiv) {
        const double w00 = ctx->delg_f32 ? (double)((float)del_g_host[0] * (float)del_g_host[0]) : del_g_host[0] * del_g_host[0];
        if (!(w00 < p.g_ord[1])) nodiv = false;
    }
    if (const char *ev = getenv("ANSFM_MERGE_WALK")) { if (!strcmp(ev, "records")) nodiv = false; }
    // a table without a boxed entry is read without the box tests (fast path only; ANSFM_LOAD_BOXTESTS=1 keeps them)
    bool nobox = nodiv && !from_k && !ctx->has_boxed;
    if (const char *ev = getenv("ANSFM_LOAD_BOXTESTS")) { if (ev[0] == '1') nobox = false; }
    // the division-free fast path in its trimmed form (kMergeOpt); ANSFM_MERGE_LEGACY=1 runs the plain form (OPT = 0): one-wave
    // blocks, the weight from its two factors, the key repacked field by field, a full list pass, the rows always a
    int opt = nodiv ? kMergeOpt : 0;
    if (const char *ev = getenv("ANSFM_MERGE_LEGACY")) { if (ev[0] == '1') opt = 0; }
    bool keys32 = nodiv && ctx->merge_keys == 32;
    if (const char *ev = getenv("ANSFM_MERGE_KEYS")) { keys32 = nodiv && atoi(ev) == 32; }
    if (keys32) opt = 0;
    // float64 weights keep the two-factor weight: the compiler contracts gd + DG[i] * DG[j] of the walk into one fma, which no
    // table of rounded products reproduces bit for bit (the float32 product is rounded before it is widened, so its table is exact)
    if (!ctx->delg_f32) opt &= ~kOptTable;
    const size_t wave_bytes = (size_t)merge_wave_rows(G, opt) * kWave * sizeof(double);
    const size_t table_bytes = (size_t)(2 * kMaxG + 2) * sizeof(double) + kMaxG * sizeof(float);
    size_t lds = keys32 ? (size_t)overlap32_lds_bytes(G, ctx->delg_f32 != 0)
                        : wave_bytes + table_bytes + (sorted ? 0 : (size_t)2 * G * kWave);
    const size_t lds_alloc = (lds + 127) / 128 * 128;      // measured (tools/calib/lds_granule.hip): 7 blocks up to 23 360 bytes
    int max_per_cu = 8;
    if (const char *ev = getenv("ANSFM_WAVES_PER_CU")) { int v = atoi(ev); if (v >= 1 && v < max_per_cu) max_per_cu = v; }
    // blocks per CU: by the LDS size rounded up to the 128-byte granule, and no more than ANSFM_WAVES_PER_CU
    long grid = 0;
    int nwaves = 1;
    if ((opt & kOptTable) != 0) {
        // one block per CU: the tables once, then as many waves' rows as the CU's 160 KiB hold (7 at G = 20), no more than
        // ANSFM_WAVES_PER_CU or the kernel's launch bound; no more blocks than the tiles need
        const size_t shared_bytes = table_bytes + weight_table_bytes(G);
        nwaves = (int)((kCuLdsBytes - shared_bytes) / wave_bytes);
        if (nwaves > max_per_cu) nwaves = max_per_cu;
        if (nwaves > kMaxBlockWaves) nwaves = kMaxBlockWaves;
        lds = shared_bytes + (size_t)nwaves * wave_bytes;
        const int rc = merge_launch_begin(ctx, p, lds, 1, {{&ctx->scratch, (size_t)nwaves * 6 * G * kWave * sizeof(double)}}, &grid);
        if (rc) return rc;
        const long ntiles = (long)n_models * (Wpad / kWave) * L;
        if (grid > (ntiles + nwaves - 1) / nwaves) grid = (ntiles + nwaves - 1) / nwaves;
    } else {
        const int rc = merge_launch_begin(ctx, p, lds_alloc, max_per_cu, {{&ctx->scratch, (size_t)6 * G * kWave * sizeof(double)}}, &grid);
        if (rc) return rc;
    }
    p.scratch = ctx->scratch.as<double>();
    // the trimmed fast path groups a wave's lanes over rows (LaneRow: the same tiles per 64-wavenumber block, so the grid and the
    // queues above hold).  64 wavenumbers of one row per wave remain for ANSFM_MERGE_LANES=wavenumbers and for a launch of 2^24
    // rows or more, whose cell numbers would leave the 32 bits lane_row computes in; bit 32 of the reported trims tells which ran
    bool lane_rows = opt != 0 && (long)n_models * L < (1L << 24);
    // the width of a row-mapped tile: 1 wavenumber x 64 rows for every shape (C2, 20 gases, the Jacobian's 696 distinct rows gain,
    // G = 10 is level: DESIGN.md 4.1), or kLaneNV x 64 / kLaneNV with ANSFM_MERGE_LANES=pairs.  Not a bit of the trims (bit 32 is
    // set for both): ansfm_last_merge_group_width reports it
    int lane_nv = 1;
    if (const char *ev = getenv("ANSFM_MERGE_LANES")) {
        if (!strcmp(ev, "wavenumbers")) lane_rows = false;
        else if (!strcmp(ev, "pairs")) lane_nv = kLaneNV;
    }
    // the instantiations with the weight table walk a wave's row-major merges without the head list (merge_rowmajor);
    // ANSFM_MERGE_ROWMAJOR=0 launches the same kernel with the walk off.  Bit 64 of the reported trims, in either lane mapping
    bool rowmajor = (opt & kOptTable) != 0;
    if (const char *ev = getenv("ANSFM_MERGE_ROWMAJOR")) { if (ev[0] == '0') rowmajor = false; }
    // a row-mapped launch on the context's own table reads the g-fastest copy where the upload built one (build_table_gfast);
    // ANSFM_TABLE_LAYOUT=wave keeps the reads of lnK.  No bit of the trims: ansfm_last_merge_table_layout reports it
    bool gfast = lane_rows && !from_k && !keys32 && ctx->lnKg_bytes != 0 && !ctx->is_lbl && W == ctx->W && Wpad == ctx->Wpad &&
                 G == ctx->G && S == ctx->S;
    if (const char *ev = getenv("ANSFM_TABLE_LAYOUT")) { if (!strcmp(ev, "wave")) gfast = false; }
    if (gfast) p.lnKg = ctx->lnKg.as<double>();
    const int flags = (lane_rows ? kFlagLaneRows : 0) | (rowmajor ? kFlagRowMajor : 0) | (gfast ? kFlagTableGfast : 0);
    ctx->merge_table_gfast = gfast ? 1 : 0;
    ctx->merge_block_waves = nwaves;
    ctx->merge_group_width = lane_rows ? lane_nv : 0;
    ctx->merge_trims = opt == 0 ? 0 : merge_opt_of(ctx->delg_f32 != 0) | (lane_rows ? kOptLaneRows : 0) | (rowmajor ? kOptRowMajor : 0);
    if (keys32) {
        HIPCHK(launch_overlap32(p, from_k, merge_list_len(G), (unsigned)grid, ctx->stream));
        return ANSFM_OK;
    }
    // a block of several waves asks for more than the 64 KiB of dynamic LDS a kernel may have without the attribute
#define LAUNCH_OPT(...)                                                                                             \
    do {                                                                                                            \
        auto kern = __VA_ARGS__;                                                                                    \
        size_t &lds_allowed = ctx->merge_lds_allowed[reinterpret_cast<const void *>(kern)];   /* 0 at first: 64 KiB */  \
        if (lds > (size_t)64 * 1024 && lds > lds_allowed) {     /* once per context (device) and instantiation */     \
            HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
            lds_allowed = lds;                                                                                      \
        }                                                                                                           \
        hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kWave * nwaves), lds, ctx->stream, p, flags, lane_nv);           \
    } while (0)
#define LAUNCH_OV2(D, FK, W32)                                                                                      \
    do {                                                                                                            \
        if (opt != 0 && nobox)                                                                                      \
            LAUNCH_OPT(k_ck_overlap<D, false, W32, true, true, true, merge_opt_of(W32)>);                           \
        else if (opt != 0)                                                                                          \
            LAUNCH_OPT(k_ck_overlap<D, FK, W32, true, true, false, merge_opt_of(W32)>);                             \
        else if (nodiv && nobox)                                                                                         \
            hipLaunchKernelGGL((k_ck_overlap<D, false, W32, true, true, true>), dim3((unsigned)grid), dim3(kWave), lds, ctx->stream, p, 0, 0); \
        else if (nodiv)                                                                                             \
            hipLaunchKernelGGL((k_ck_overlap<D, FK, W32, true, true>), dim3((unsigned)grid), dim3(kWave), lds, ctx->stream, p, 0, 0); \
        else if (sorted)                                                                                            \
            hipLaunchKernelGGL((k_ck_overlap<D, FK, W32, true>), dim3((unsigned)grid), dim3(kWave), lds, ctx->stream, p, 0, 0);  \
        else                                                                                                        \
            hipLaunchKernelGGL((k_ck_overlap<D, FK, W32, false>), dim3((unsigned)grid), dim3(kWave), lds, ctx->stream, p, 0, 0); \
    } while (0)
#define LAUNCH_OV(D, FK)                                                                              \
    do {                                                                                              \
        if (ctx->delg_f32) LAUNCH_OV2(D, FK, true); else LAUNCH_OV2(D, FK, false);                    \
    } while (0)
#define LAUNCH_OVN(FK)                                                \
    switch (merge_list_len(G)) {                                      \
        case 8: LAUNCH_OV(8, FK); break;                              \
        case 10: LAUNCH_OV(10, FK); break;                            \
        case 16: LAUNCH_OV(16, FK); break;                            \
        case 20: LAUNCH_OV(20, FK); break;                            \
        default: LAUNCH_OV(32, FK); break;                            \
    }
    if (from_k) { LAUNCH_OVN(true); } else { LAUNCH_OVN(false); }
#undef LAUNCH_OVN
#undef LAUNCH_OV
#undef LAUNCH_OV2
#undef LAUNCH_OPT
    HIPCHK(hipGetLastError());
    return ANSFM_OK;
}

}  // namespace ansfm

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
    // eight tile queues, then the forward merge's 64-bit totals (ansfm_last_merge_rowmajor, _order, _suffix): cleared by one memset
    p.tile_counter = reinterpret_cast<unsigned int *>(ctx->d_flag.as<int>() + kFlagTileCounter);
    p.W = W; p.Wpad = Wpad; p.G = G; p.NT = ctx->NT; p.S = S; p.L = L; p.n_models = n_models;
    p.delg_f32 = ctx->delg_f32;
    merge_g_ord(del_g_host, G, ctx->delg_f32 != 0, p.g_ord);
}

int merge_launch_begin(ansfm_ctx *ctx, const OverlapParams &p, long grid, std::initializer_list<MergeWorkspace> workspaces)
{
    for (const MergeWorkspace &w : workspaces) HIPCHK(w.buf->reserve((size_t)grid * w.bytes_per_block));
    HIPCHK(hipMemsetAsync(p.tile_counter, 0, (8 + 2 * kMergeTotals) * sizeof(unsigned int), ctx->stream));
    return ANSFM_OK;
}

// The 100 instantiations of k_ck_overlap, 10 per (list length, W32), and which of them a plan names.  The box-free loads are
// compiled with FROM_K = false only (the seam reads no table) and serve both values of from_k.  The kernels appear in the
// code object in the order they are first named here, FROM_K = true first, then by list length and weight type.
using MergeKernel = void (*)(OverlapParams, int, int);

template <int D, bool FK, bool W32>
static MergeKernel overlap_kernel_of(const MergePlan &m)
{
    // the trims this weight type is compiled with: the weight table only with float32 weights (merge_plan)
    constexpr int kTrimmed = W32 ? kMergeOpt : (kMergeOpt & ~kOptTable);
    if (m.opt == kTrimmed) return m.nobox ? k_ck_overlap<D, false, W32, true, true, true, kTrimmed> : k_ck_overlap<D, FK, W32, true, true, false, kTrimmed>;
    if (m.opt != 0) return nullptr;
    if (m.nodiv) return m.nobox ? k_ck_overlap<D, false, W32, true, true, true> : k_ck_overlap<D, FK, W32, true, true>;
    return m.sorted ? k_ck_overlap<D, FK, W32, true> : k_ck_overlap<D, FK, W32, false>;
}

template <bool FK>
static MergeKernel overlap_kernel_fk(const MergePlan &m, bool w32, int G)
{
    return by_list_len(G, [&](auto d) {
        constexpr int D = decltype(d)::value;
        return w32 ? overlap_kernel_of<D, FK, true>(m) : overlap_kernel_of<D, FK, false>(m);
    });
}

static MergeKernel overlap_kernel(const MergePlan &m, bool from_k, bool w32, int G)
{
    return from_k ? overlap_kernel_fk<true>(m, w32, G) : overlap_kernel_fk<false>(m, w32, G);
}

int launch_overlap(ansfm_ctx *ctx, bool from_k, const double *kin, int W, int Wpad, int G, int S,
                   int L, int n_models, const LayerInterp *li, const double *amount,
                   const double *del_g_dev, const double *del_g_host, double *tau, bool generic)
{
    OverlapParams p;
    memset(&p, 0, sizeof p);
    merge_params(ctx, p, kin, W, Wpad, G, S, L, n_models, li, amount, del_g_dev, del_g_host, tau);
    const bool w32 = ctx->delg_f32 != 0;
    MergeCall c;
    c.from_k = from_k; c.generic = generic; c.monotone = ctx->monotone != 0; c.has_boxed = ctx->has_boxed != 0; c.delg_f32 = w32;
    c.merge_keys = ctx->merge_keys;
    c.G = G; c.S = S; c.W = W; c.Wpad = Wpad; c.L = L; c.n_models = n_models; c.num_cus = ctx->num_cus;
    c.w00 = w32 ? (double)((float)del_g_host[0] * (float)del_g_host[0]) : del_g_host[0] * del_g_host[0];
    c.g_ord1 = p.g_ord[1];
    c.gfast_copy = ctx->lnKg_bytes != 0 && !ctx->is_lbl;
    c.table_W = ctx->W; c.table_Wpad = ctx->Wpad; c.table_G = ctx->G; c.table_S = ctx->S;
    c.lds32 = overlap32_lds_bytes(G, w32);
    // the schedule of a whole walk from the launch's own g_ord; the table kernels alone read it (float32 weights)
    if (w32) merge_static_build(del_g_host, p.g_ord, G, p.st);
    c.static_valid = p.st.valid != 0;
    const MergePlan m = merge_plan(c, merge_switches_from_env());

    const int rc = merge_launch_begin(ctx, p, m.grid, {{&ctx->scratch, m.scratch_bytes_per_block}});
    if (rc) return rc;
    p.scratch = ctx->scratch.as<double>();
    if (m.gfast) p.lnKg = ctx->lnKg.as<double>();
    ctx->last_merge = m;
    ctx->last_merge_G = G;
    ctx->last_merge_ordered = false;
    ansfm_ctx::MergeHintKey key;
    bool valid = false;
    if (m.order) {
        // the pattern bytes of the launch before, if it was a launch of this key; else zeros, which are the identity order
        key.source = from_k ? 0 : ctx->table_generation;
        key.W = W; key.Wpad = Wpad; key.R = n_models * L; key.S = S; key.G = G;
        HIPCHK(ctx->merge_hint.reserve((size_t)2 * Wpad));
        valid = key == ctx->merge_hint_key;
        if (!valid) HIPCHK(hipMemsetAsync(ctx->merge_hint.p, 0, (size_t)2 * Wpad, ctx->stream));
        p.hint_in = ctx->merge_hint.as<unsigned char>() + (size_t)ctx->merge_hint_parity * Wpad;
        p.hint_out = ctx->merge_hint.as<unsigned char>() + (size_t)(1 - ctx->merge_hint_parity) * Wpad;
    }
    if (m.keys32) {
        HIPCHK(launch_overlap32(p, from_k, (unsigned)m.grid, ctx->stream));
        return ANSFM_OK;
    }
    const MergeKernel kern = overlap_kernel(m, from_k, w32, G);
    if (!kern) FAIL(ANSFM_ERR_UNSUPPORTED, "forward merge: no kernel is compiled for this plan");
    // a block of several waves asks for more than the 64 KiB of dynamic LDS a kernel may have without the attribute:
    // raised once per context (device) and instantiation
    if (m.lds > (size_t)64 * 1024) {
        size_t &lds_allowed = ctx->merge_lds_allowed[reinterpret_cast<const void *>(kern)];      // 0 at first: 64 KiB
        if (m.lds > lds_allowed) {
            HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)m.lds));
            lds_allowed = m.lds;
        }
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)m.grid), dim3(kWave * m.nwaves), m.lds, ctx->stream, p, m.flags, m.lane_nv);
    HIPCHK(hipGetLastError());
    if (m.order) {
        ctx->merge_hint_parity ^= 1;            // the next launch reads what this one writes
        ctx->merge_hint_key = key;
        ctx->last_merge_ordered = valid;
    }
    return ANSFM_OK;
}

}  // namespace ansfm

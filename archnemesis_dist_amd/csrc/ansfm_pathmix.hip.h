// ansfm_pathmix.hip.h -- the host side the fused gradient entries share (ansfm_transit.hip, ansfm_occultation.hip,
// ansfm_limb.hip, ansfm_disc.hip): the checks of the paths and of the mixing matrix, the path matrix, the prologue of a call, the reservation
// of dMOD, the staged call around an entry's own launcher, and what stands behind ansfm_*_last.  A helper that can refuse takes
// the entry's name (`what`, "cirsradg_ck_...") and formats it into the message.  Inline functions only; no kernel here.
#pragma once
#include "ansfm_ctx.hip.h"
#include "ansfm_pathmix_kernels.hip.h"
#include "ansfm_rt_params.h"

namespace ansfm {

inline int ensure_events(ansfm_ctx *ctx, FusedRoute &route)
{
    for (hipEvent_t &e : route.ev)
        if (!e) HIPCHK(hipEventCreate(&e));
    return ANSFM_OK;
}

// ansfm_<name>_last: the scratch bytes of the route's last call and the times between its three events
inline int fused_last(const ansfm_ctx *cctx, FusedRoute ansfm_ctx::*member, double info[3], const char *name)
{
    ansfm_ctx *ctx = const_cast<ansfm_ctx *>(cctx);
    CHECK_CTX(ctx);
    const FusedRoute &route = ctx->*member;
    if (!info) FAIL(ANSFM_ERR_INVALID, std::string(name) + "_last: null argument");
    if (!route.recorded) FAIL(ANSFM_ERR_INVALID, std::string(name) + "_last: no ansfm_cirsradg_ck_" + name + " call recorded yet");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipEventSynchronize(route.ev[2]));
    float a = 0.f, b = 0.f;
    HIPCHK(hipEventElapsedTime(&a, route.ev[0], route.ev[1]));
    HIPCHK(hipEventElapsedTime(&b, route.ev[1], route.ev[2]));
    info[0] = (double)route.scratch_bytes;
    info[1] = a;
    info[2] = b;
    return ANSFM_OK;
}

// more than the 64 KiB of dynamic LDS a kernel may have without the attribute
template <class Kernel> inline int allow_lds(ansfm_ctx *ctx, Kernel kernel, size_t bytes)
{
    if (bytes > (size_t)64 * 1024)
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMixLdsOneBlock));
    return ANSFM_OK;
}

// NLAYIN [P] within 0 .. LIMAX and the entries j < NLAYIN[p] of LAYINC [LIMAX][P] within 0 .. L - 1; padding is never read
inline int check_paths(ansfm_ctx *ctx, const char *what, int L, int P, int LIMAX, const int32_t *NLAYIN, const int32_t *LAYINC)
{
    for (int p = 0; p < P; ++p) {
        if (NLAYIN[p] < 0 || NLAYIN[p] > LIMAX) FAIL(ANSFM_ERR_INVALID, std::string(what) + ": NLAYIN outside 0 .. LIMAX");
        for (int j = 0; j < NLAYIN[p]; ++j)
            if (LAYINC[(size_t)j * P + p] < 0 || LAYINC[(size_t)j * P + p] >= L)
                FAIL(ANSFM_ERR_INVALID, std::string(what) + ": LAYINC outside 0 .. L - 1");
    }
    return ANSFM_OK;
}

// The mixing matrix C (Q, P) by rows: mix_ptr [Q + 1] from 0 and not decreasing, mix_path within 0 .. P - 1
inline int check_mix(ansfm_ctx *ctx, const char *what, int P, int Q, const int32_t *mix_ptr, const int32_t *mix_path,
                     const double *mix_val, size_t *mnz_out)
{
    if (mix_ptr[0] != 0) FAIL(ANSFM_ERR_INVALID, std::string(what) + ": mix_ptr[0] must be 0");
    for (int q = 0; q < Q; ++q)
        if (mix_ptr[q + 1] < mix_ptr[q]) FAIL(ANSFM_ERR_INVALID, std::string(what) + ": mix_ptr must not decrease");
    const size_t mnz = (size_t)mix_ptr[Q];
    if (mnz && (!mix_path || !mix_val)) FAIL(ANSFM_ERR_INVALID, std::string(what) + ": null mix_path / mix_val");
    for (size_t i = 0; i < mnz; ++i)
        if (mix_path[i] < 0 || mix_path[i] >= P) FAIL(ANSFM_ERR_INVALID, std::string(what) + ": mix_path outside 0 .. P - 1");
    *mnz_out = mnz;
    return ANSFM_OK;
}

// The path matrix Sm[l][p] = sum of SCALE over the entries j < NLAYIN[p] of path p with LAYINC[j][p] = l (checked paths), dense
// with the mask of what some entry touched, and compressed by path: col_ptr [P + 1], col_lay [nnz], col_val [nnz]
struct PathMatrix {
    std::vector<double> Sm, col_val;       // Sm [L][P]
    std::vector<char> hit;                 // [L][P]
    std::vector<int32_t> col_ptr, col_lay;
    size_t nnz = 0;
};
inline PathMatrix build_path_matrix(int L, int P, const int32_t *NLAYIN, const int32_t *LAYINC, const double *SCALE)
{
    PathMatrix m;
    m.Sm.assign((size_t)L * P, 0.0);
    m.hit.assign((size_t)L * P, 0);
    for (int p = 0; p < P; ++p)
        for (int j = 0; j < NLAYIN[p]; ++j) {
            const int l = LAYINC[(size_t)j * P + p];
            m.Sm[(size_t)l * P + p] += SCALE[(size_t)j * P + p];
            m.hit[(size_t)l * P + p] = 1;
        }
    for (int p = 0; p < P; ++p) {
        m.col_ptr.push_back((int32_t)m.col_lay.size());
        for (int l = 0; l < L; ++l)
            if (m.hit[(size_t)l * P + p]) { m.col_lay.push_back(l); m.col_val.push_back(m.Sm[(size_t)l * P + p]); }
    }
    m.col_ptr.push_back((int32_t)m.col_lay.size());
    m.nnz = m.col_lay.size();
    return m;
}

// What follows an entry's own argument checks, up to the point where everything that can refuse the arguments has: q zeroed but
// for the gas selection and the merge slot behind every parameter; with grad_kernel, the slot chunk of the contraction (*SC,
// *lds_grad) and the cap on wavenumber tiles; the pending shared gas gradient; then the device is selected and what the last
// call left for ansfm_map2pro and ansfm_*_last is withdrawn.
template <class Params>
inline int fused_prologue(ansfm_ctx *ctx, const char *what, FusedRoute &route, int L, const int32_t *igas_map, int NVMR, int NPAR,
                          Params &q, const char *grad_kernel = nullptr, int *SC = nullptr, size_t *lds_grad = nullptr)
{
    memset(&q, 0, sizeof q);
    q.gas_mask = ctx->is_lbl ? 0xFFFFFFFFu : ctx->grad_gas_mask;
    int rc;
    if ((rc = fill_slot_of_param(ctx, igas_map, NVMR, NPAR, q.gas_mask, q.slot_of_param))) return rc;
    if (grad_kernel) {
        if (!(*SC = slab_chunk(ctx->G, ctx->S + 1, lds_grad)))
            FAIL(ANSFM_ERR_UNSUPPORTED, std::string(what) + ": too many g-ordinates for the LDS of " + grad_kernel);
        if (ctx->Wpad / kWave > 65535)
            FAIL(ANSFM_ERR_UNSUPPORTED, std::string(what) + ": more than 65535 wavenumber tiles (4.19e6 wavenumbers)");
    }
    if (ctx->dcont_gas_L && ctx->dcont_gas_L != L) {
        ctx->dcont_gas_L = 0;
        FAIL(ANSFM_ERR_INVALID, std::string(what) + ": the pending shared gas gradient (ansfm_set_shared_gas_gradient) is for a "
                                                    "different number of layers");
    }
    HIPCHK(hipSetDevice(ctx->device));
    ctx->dspec_dims[0] = 0;
    route.recorded = 0;
    return ANSFM_OK;
}

// dMOD as a whole in dspec_ref: 8 W NPAR L Q bytes (*n_dmod elements).  A reservation that fails, or `refuse` (a size of the
// entry's own that overflows), is the caller's cue to take the un-collapsed route.
inline int reserve_dmod(ansfm_ctx *ctx, const char *what, int NPAR, int L, int Q, bool refuse, size_t *n_dmod)
{
    const size_t D = sizeof(double);
    if (refuse || __builtin_mul_overflow((size_t)ctx->W * NPAR, (size_t)L * Q, n_dmod) || *n_dmod > SIZE_MAX / D ||
        ctx->dspec_ref.reserve(*n_dmod * D) != hipSuccess) {
        (void)hipGetLastError();
        FAIL(ANSFM_ERR_UNSUPPORTED, std::string(what) + ": dMOD (8 W NPAR L Q bytes) could not be reserved on the device");
    }
    return ANSFM_OK;
}

// The device side of a fused call.  Staged through ctx->hb[] in this order: the five layer arrays, the entry's hd and hi, xfac
// (or nullptr); then the gas stage (grad_gas_stage, which stages nothing).  fill(staged, copies) sets up the entry's params and
// lists the device -> host copies of its results (a null dst is skipped); launch() runs the entry's kernels between ev[2] and
// ev[3].  Then the copies are queued and check_unsorted synchronises.  hd / hi / the copies' host side belong to the caller's
// frame: on any failure the stream is synchronised before the return, so that whatever was queued from them has run before
// they go.  On success dspec_dims = (W, NPAR, L, Q) and the route's call is recorded.
struct FusedStaged {
    const double *cont_t, *dcont_t;   // the continuum and its gradients in the wave-fastest layouts, or nullptr
    const double *dcont_gas;          // the shared gas gradient pending for this call (consumed), or nullptr
    const double *dd, *xfac;          // hd and xfac on the device
    const int32_t *di;                // hi on the device
};
struct FusedCopy {
    void *dst;
    const void *src;
    size_t bytes;
};
template <class Fill, class Launch>
inline int fused_staged_call(ansfm_ctx *ctx, FusedRoute &route, int L, const double *lay_press_pa, const double *lay_temp,
                             const double *amount, const double *taucont, const double *dtaucon, int NPAR, int Q,
                             const std::vector<double> &hd, const std::vector<int32_t> &hi, const double *xfac, Fill fill, Launch launch)
{
    const int W = ctx->W, S = ctx->S;
    auto on_device = [&]() -> int {
        Stager st{ctx};
        const double *press = st.up(lay_press_pa, L), *temp = st.up(lay_temp, L), *am = st.up(amount, (size_t)L * S),
                     *cont = st.up(taucont, (size_t)L * W), *dcont = st.up(dtaucon, (size_t)L * W * NPAR);
        FusedStaged s{};
        s.dd = st.up(hd.data(), hd.size());
        s.di = st.up(hi.data(), hi.size());
        s.xfac = st.up(xfac, W);
        if (st.rc) return st.rc;
        int rc;
        if ((rc = grad_gas_stage(ctx, 1, L, press, temp, am, cont, dcont, NPAR, &s.cont_t, &s.dcont_t))) return rc;
        if (ctx->dcont_gas_L) s.dcont_gas = ctx->dcont_gas.as<double>();
        std::vector<FusedCopy> copies;
        if ((rc = fill(s, copies))) return rc;
        ctx->dcont_gas_L = 0;                   // one call only
        HIPCHK(hipEventRecord(ctx->ev[2], ctx->stream));
        if ((rc = launch())) return rc;
        HIPCHK(hipEventRecord(ctx->ev[3], ctx->stream));
        call_recorded(ctx, 1, L);
        for (const FusedCopy &c : copies)
            if (c.dst) HIPCHK(hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, ctx->stream));
        return check_unsorted(ctx);             // synchronises
    };
    if (int rc = on_device()) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    ctx->dspec_dims[0] = W; ctx->dspec_dims[1] = NPAR; ctx->dspec_dims[2] = L; ctx->dspec_dims[3] = Q;
    route.recorded = 1;
    return ANSFM_OK;
}

}  // namespace ansfm

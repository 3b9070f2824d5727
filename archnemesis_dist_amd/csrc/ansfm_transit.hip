// ansfm_transit.hip -- translation unit of the transit kernels (ansfm_transit_kernels.hip.h): the launcher the entry point
// ansfm_cirsradg_ck_transit of ansfm_api.hip calls, and ansfm_transit_last.  gfx950 only.
#include "ansfm_transit_kernels.hip.h"
#include "ansfm_ctx.hip.h"

namespace ansfm {

// k_transit_sens, then k_transit_grad, on ctx->stream, between the events transit_last reads
int launch_transit(ansfm_ctx *ctx, const TransitParams &q)
{
    const int rows = std::max(q.L, q.P);
    if (rows > kTransitMaxRows) FAIL(ANSFM_ERR_UNSUPPORTED, "transit: more than 320 layers or paths (the 160 KiB LDS tile of k_transit_sens)");
    if (q.Wpad / kWave > 65535) FAIL(ANSFM_ERR_UNSUPPORTED, "transit: more than 65535 wavenumber tiles (4.19e6 wavenumbers)");
    for (hipEvent_t &e : ctx->transit_ev)
        if (!e) HIPCHK(hipEventCreate(&e));
    const unsigned tiles = (unsigned)(q.Wpad / kWave);
    HIPCHK(hipEventRecord(ctx->transit_ev[0], ctx->stream));
    hipLaunchKernelGGL(k_transit_sens, dim3(tiles, (unsigned)q.G), dim3(kWave), (size_t)rows * kWave * sizeof(double), ctx->stream, q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->transit_ev[1], ctx->stream));
    hipLaunchKernelGGL(k_transit_grad, dim3(tiles, (unsigned)rows), dim3(kWave), (size_t)(q.G + q.NP1) * kWave * sizeof(double),
                       ctx->stream, q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->transit_ev[2], ctx->stream));
    return ANSFM_OK;
}

}  // namespace ansfm

using namespace ansfm;

extern "C" {

int ansfm_transit_last(const ansfm_ctx *cctx, double info[3])
{
    ansfm_ctx *ctx = const_cast<ansfm_ctx *>(cctx);
    CHECK_CTX(ctx);
    if (!info) FAIL(ANSFM_ERR_INVALID, "transit_last: null argument");
    if (!ctx->transit_recorded) FAIL(ANSFM_ERR_INVALID, "transit_last: no ansfm_cirsradg_ck_transit call recorded yet");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipEventSynchronize(ctx->transit_ev[2]));
    float a = 0.f, b = 0.f;
    HIPCHK(hipEventElapsedTime(&a, ctx->transit_ev[0], ctx->transit_ev[1]));
    HIPCHK(hipEventElapsedTime(&b, ctx->transit_ev[1], ctx->transit_ev[2]));
    info[0] = (double)ctx->transit_scratch_bytes;
    info[1] = a;
    info[2] = b;
    return ANSFM_OK;
}

}  // extern "C"

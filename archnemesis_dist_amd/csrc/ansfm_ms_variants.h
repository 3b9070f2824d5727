// ansfm_ms_variants.h -- per-model phase functions inside the multiple-scattering batch (ansfm_set_phase_variants), planned on
// the host from integers and the bits of the phase arrays alone: the validation of a pending setting against the call that
// consumes it, which (variant, component) pairs differ from variant 0, the list of pairs one launch of k_ms_phase /
// k_ms_hansen_seq covers, and where a variant's phase matrices and Hansen factors lie.  No HIP header: a plain C++17 compiler
// builds it (tests/host/ms_variants_main.cpp).  DESIGN.md 4.4f.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

namespace ansfm {

// What ansfm_set_phase_variants leaves in the context: copies of the caller's arrays, taken at set time.
struct MsVariantSet {
    int n_models = 0, V = 1, ncont = 0, nth = 0;
    std::vector<int32_t> phase_of;       // [n_models]
    std::vector<double> phasarr;         // [V - 1][ncont][W][2][nth]: variants 1 .. V-1 (variant 0 is the call's phasarr)
    bool armed() const { return V > 1; }
};

// 0: the setting fits a call of n_models models, ncont populations and nth angles; else why it does not (ANSFM_ERR_INVALID)
inline int ms_variants_validate(const MsVariantSet &s, int n_models, int ncont, int nth, std::string *why)
{
    auto bad = [&](const std::string &m) { if (why) *why = m; return 1; };
    if (s.n_models != n_models)
        return bad("set for n_models = " + std::to_string(s.n_models) + ", the call has " + std::to_string(n_models));
    if (s.ncont != ncont) return bad("set for ncont = " + std::to_string(s.ncont) + ", the call has " + std::to_string(ncont));
    if (s.nth != nth) return bad("set for nth = " + std::to_string(s.nth) + ", the call has " + std::to_string(nth));
    if ((int)s.phase_of.size() != n_models) return bad("phase_of does not hold n_models entries");
    for (int m = 0; m < n_models; ++m)
        if (s.phase_of[m] < 0 || s.phase_of[m] >= s.V)
            return bad("phase_of[" + std::to_string(m) + "] = " + std::to_string(s.phase_of[m]) + " is outside [0, V = " +
                       std::to_string(s.V) + ")");
    if (n_models > 0 && s.phase_of[0] != 0) return bad("phase_of[0] must be 0: variant 0 is the call's phasarr");
    return 0;
}

// The layout and the launches of a call with V variants.  A variant's phase matrices and factors keep variant 0's layout,
// ppl / pmi [W][nf + 1][ncomp][nn] and fc [G][W][ncomp][nn], one variant after the other:
//   [V][ ppl (nph) | pmi (nph) | fc (nfc) ]      (doubles; variant v at v * vstride)
// so a reader adds v * vstride to each of variant 0's three pointers.  Components that do not differ from variant 0's --
// Rayleigh always -- are copied from variant 0 on the device, never integrated or walked again.
struct MsVariantPlan {
    int V = 1, ncont = 0, ncomp = 1;
    size_t nph = 0, nfc = 0, vstride = 0, total = 0;     // doubles; total = V * vstride
    size_t st_phas = 0;                                   // doubles between two variants' phasarr: ncont * W * 2 * nth
    std::vector<unsigned char> diff;                      // [V][ncomp]: the component's phasarr differs from variant 0's in some bit
    std::vector<int32_t> pairs;                           // [npairs][2] (variant, component): variant 0's components in use
    int npairs0 = 0, npairs = 0;                          // first (aerosols, then Rayleigh with iray > 0), then the differing ones
    size_t ppl_off(int v) const { return (size_t)v * vstride; }
    size_t pmi_off(int v) const { return (size_t)v * vstride + nph; }
    size_t fc_off(int v) const { return (size_t)v * vstride + 2 * nph; }
    size_t bytes_variants() const { return (size_t)(V - 1) * vstride * sizeof(double); }
    int ndiff(int v) const { int n = 0; for (int c = 0; c < ncomp; ++c) n += diff[(size_t)v * ncomp + c]; return n; }
};

// phasarr0 [ncont][W][2][nth]; variants [V - 1][ncont][W][2][nth] (unused with V = 1); nmu: the streams the kernels run on
// (16 for a padded quadrature)
inline MsVariantPlan ms_variants_plan(int V, int ncont, int iray, size_t W, int nth, int nf, int nmu, int G, const double *phasarr0,
                                      const double *variants)
{
    MsVariantPlan pl;
    pl.V = V; pl.ncont = ncont; pl.ncomp = ncont + 1;
    const size_t nn = (size_t)nmu * nmu, per_c = W * 2 * (size_t)nth;
    pl.nph = W * (size_t)(nf + 1) * pl.ncomp * nn;
    pl.nfc = (size_t)G * W * pl.ncomp * nn;
    pl.vstride = 2 * pl.nph + pl.nfc;
    pl.total = (size_t)V * pl.vstride;
    pl.st_phas = (size_t)ncont * per_c;
    pl.diff.assign((size_t)V * pl.ncomp, 0);
    for (int c = 0; c < ncont; ++c) { pl.pairs.push_back(0); pl.pairs.push_back(c); }
    if (iray > 0) { pl.pairs.push_back(0); pl.pairs.push_back(ncont); }
    pl.npairs0 = (int)pl.pairs.size() / 2;
    for (int v = 1; v < V; ++v)
        for (int c = 0; c < ncont; ++c) {
            const double *a = variants + (size_t)(v - 1) * pl.st_phas + (size_t)c * per_c;
            if (memcmp(a, phasarr0 + (size_t)c * per_c, per_c * sizeof(double)) != 0) {
                pl.diff[(size_t)v * pl.ncomp + c] = 1;
                pl.pairs.push_back(v); pl.pairs.push_back(c);
            }
        }
    pl.npairs = (int)pl.pairs.size() / 2;
    return pl;
}

}  // namespace ansfm

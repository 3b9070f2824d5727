// ms_variants_main.cpp -- runs the host planning of per-model phase functions (csrc/ansfm_ms_variants.h) on cases read from
// standard input, one per line, and prints what it planned (tests/test_ms_variants_host.py compares with NumPy).
//   name V ncont iray W nth nf nmu G  set_n set_ncont set_nth  call_n call_ncont call_nth  phase_of[set_n]  tags[V * ncont]
//        npert (v c index hexvalue) * npert
// Variant v's block of population c, [W][2][nth], is filled with the number tags[v * ncont + c]; a perturbation then sets one of
// its elements.  Built by a plain C++17 compiler under AddressSanitizer and UBSan: the arrays have exactly the planned sizes.
#include <stdio.h>
#include <stdlib.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "ansfm_ms_variants.h"

using namespace ansfm;

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string name;
        int V, ncont, iray, W, nth, nf, nmu, G, call_n, call_ncont, call_nth;
        MsVariantSet s;
        in >> name >> V >> ncont >> iray >> W >> nth >> nf >> nmu >> G >> s.n_models >> s.ncont >> s.nth >> call_n >> call_ncont >> call_nth;
        s.V = V;
        s.phase_of.resize((size_t)s.n_models);
        for (auto &v : s.phase_of) in >> v;
        const size_t per_c = (size_t)W * 2 * nth, per_v = per_c * ncont;
        std::vector<double> all((size_t)V * per_v);
        for (int v = 0; v < V; ++v)
            for (int c = 0; c < ncont; ++c) {
                double tag;
                in >> tag;
                for (size_t i = 0; i < per_c; ++i) all[(size_t)v * per_v + (size_t)c * per_c + i] = tag;
            }
        int npert = 0;
        in >> npert;
        for (int k = 0; k < npert; ++k) {
            int v, c;
            size_t idx;
            std::string hex;
            in >> v >> c >> idx >> hex;
            all[(size_t)v * per_v + (size_t)c * per_c + idx] = strtod(hex.c_str(), nullptr);
        }
        if (!in) { fprintf(stderr, "bad case line: %s\n", line.c_str()); return 2; }
        std::vector<double> v0(all.begin(), all.begin() + (long)per_v);
        s.phasarr.assign(all.begin() + (long)per_v, all.end());           // exactly [V - 1][ncont][W][2][nth]
        std::string why;
        const int bad = ms_variants_validate(s, call_n, call_ncont, call_nth, &why);
        printf("%s valid=%d armed=%d", name.c_str(), bad ? 0 : 1, s.armed() ? 1 : 0);
        if (!bad) {
            const MsVariantPlan pl = ms_variants_plan(V, ncont, iray, (size_t)W, nth, nf, nmu, G, v0.data(), s.phasarr.data());
            printf(" npairs0=%d npairs=%d pairs=", pl.npairs0, pl.npairs);
            for (int k = 0; k < pl.npairs; ++k) printf("%s%d:%d", k ? "," : "", pl.pairs[2 * k], pl.pairs[2 * k + 1]);
            printf(" diff=");
            for (unsigned char d : pl.diff) printf("%d", (int)d);
            printf(" nph=%zu nfc=%zu vstride=%zu total=%zu st_phas=%zu bytes=%zu off=", pl.nph, pl.nfc, pl.vstride, pl.total, pl.st_phas,
                   pl.bytes_variants());
            for (int v = 0; v < V; ++v) printf("%s%zu:%zu:%zu", v ? "," : "", pl.ppl_off(v), pl.pmi_off(v), pl.fc_off(v));
            printf(" ndiff=");
            for (int v = 0; v < V; ++v) printf("%s%d", v ? "," : "", pl.ndiff(v));
        }
        printf("\n");
    }
    return 0;
}

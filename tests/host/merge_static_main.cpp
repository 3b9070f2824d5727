// merge_static_main.cpp -- prints the static schedule of a whole row-major walk (merge_static_build, csrc/ansfm_merge_plan.h)
// for the weights it reads from standard input, one case per line: a name, then the G values of del_g (anything strtod reads:
// hexadecimal floats, "nan").  g_ord is formed as the launcher forms it for float32 weights (merge_g_ord).  One line per case:
//   name valid=V nbins=N gd_end=H last_width=H masks=M0,M1,.. c1=H,H,.. c2=H,H,..
// doubles as hexadecimal floats, so that the reader compares bits.  Host code only: tests/test_merge_static_model.py builds it
// with the host compiler and its sanitizers.
#include <stdio.h>
#include <stdlib.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "ansfm_merge_plan.h"

using namespace ansfm;

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream words(line);
        std::string name, word;
        if (!(words >> name)) continue;
        std::vector<double> del_g;
        while (words >> word) del_g.push_back(strtod(word.c_str(), nullptr));
        const int G = (int)del_g.size();
        if (G < 1 || G > kMaxG) { fprintf(stderr, "%s: %d weights\n", name.c_str(), G); return 2; }
        double g_ord[kMaxG + 2];
        merge_g_ord(del_g.data(), G, true, g_ord);
        MergeStatic s;
        merge_static_build(del_g.data(), g_ord, G, s);
        printf("%s valid=%d nbins=%d gd_end=%a last_width=%a masks=", name.c_str(), s.valid, s.nbins, s.gd_end, s.last_width);
        for (int i = 0; i < G; ++i) printf("%s%u", i ? "," : "", s.rowmask[i]);
        printf(" c1=");
        for (int b = 0; b < s.nbins; ++b) printf("%s%a", b ? "," : "", s.c1[b]);
        printf(" c2=");
        for (int b = 0; b < s.nbins; ++b) printf("%s%a", b ? "," : "", s.c2[b]);
        printf("\n");
    }
    return 0;
}

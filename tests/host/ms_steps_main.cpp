// ms_steps_main.cpp -- runs the shared steps of the multiple-scattering chains (csrc/ansfm_ms_chain_steps.h) on the cases it
// reads from standard input, one per line: a name, the step, its arguments as numbers.  Prints the name and `field=value` with
// doubles in hexadecimal, so that the test compares bits.  Host code only: tests/test_ms_steps_host.py builds it with the host
// compiler and its sanitizers.
#include <math.h>
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "ansfm_ms_chain_steps.h"

using namespace ansfm;

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream words(line);
        std::string name, step;
        if (!(words >> name >> step)) continue;
        std::vector<double> a;
        for (std::string w; words >> w;) a.push_back(std::stod(w));
        printf("%s", name.c_str());
        if (step == "scalars" && a.size() == 3) {
            const MsLayerScalars s = ms_layer_scalars(a[0], a[1], a[2]);
            printf(" tauscat=%a omega=%a kind=%d", s.tauscat, s.omega, (int)s.kind);
        } else if (step == "doubling" && a.size() == 5) {
            const MsDoublingStart d = ms_doubling_start(a[0], a[1], a[2], a[3], (int)a[4], [](double x) { return log2(x); },
                                                        [](double x) { return exp2(x); });
            printf(" con=%a nd=%d tau0=%a fr=%a fs=%a", d.con, d.nd, d.tau0, d.fr, d.fs);
        } else if (step == "bracket" && a.size() >= 4) {          // nq, z, then every slot of the quadrature
            const int nq = (int)a[0];
            const std::vector<double> mu(a.begin() + 2, a.end());
            if (nq < 2 || (size_t)nq > mu.size()) { printf(" error=nq\n"); return 1; }
            printf(" bracket=%d", ms_bracket(mu.data(), nq, a[1]));
        } else if (step == "bilinear" && a.size() == 6) {
            printf(" value=%a", ms_bilinear(a.data(), a[4], a[5]));
        } else if (step == "fourier" && !a.empty()) {
            double rad = 0.0;
            bool conv1 = false;
            int used = 0;
            for (double d : a) {
                ++used;
                if (ms_fourier_step(d, rad, conv1)) break;
            }
            printf(" rad=%a terms=%d", rad, used);
        } else {
            printf(" error=step\n");
            return 1;
        }
        printf("\n");
    }
    return 0;
}

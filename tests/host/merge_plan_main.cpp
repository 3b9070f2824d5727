// merge_plan_main.cpp -- prints the forward merge's launch plan (csrc/ansfm_merge_plan.h) for the calls it reads from standard
// input, one per line: a name, then `field=value` for the fields of MergeCall and `ANSFM_...=value` for switches, which are
// put into the environment for that line and read back by merge_switches_from_env.  Host code only: tests/test_merge_plan_host.py
// builds it with the host compiler and its sanitizers.
#include <stdio.h>

#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "ansfm_merge_plan.h"

using namespace ansfm;

static bool set_field(MergeCall &c, const std::string &key, const std::string &val)
{
    const std::map<std::string, bool MergeCall::*> flags = {
        {"from_k", &MergeCall::from_k}, {"generic", &MergeCall::generic}, {"monotone", &MergeCall::monotone},
        {"has_boxed", &MergeCall::has_boxed}, {"delg_f32", &MergeCall::delg_f32}, {"gfast_copy", &MergeCall::gfast_copy}};
    const std::map<std::string, int MergeCall::*> ints = {
        {"merge_keys", &MergeCall::merge_keys}, {"G", &MergeCall::G}, {"S", &MergeCall::S}, {"W", &MergeCall::W},
        {"Wpad", &MergeCall::Wpad}, {"L", &MergeCall::L}, {"n_models", &MergeCall::n_models}, {"num_cus", &MergeCall::num_cus},
        {"table_W", &MergeCall::table_W}, {"table_Wpad", &MergeCall::table_Wpad}, {"table_G", &MergeCall::table_G},
        {"table_S", &MergeCall::table_S}};
    if (flags.count(key)) c.*flags.at(key) = std::stoi(val) != 0;
    else if (ints.count(key)) c.*ints.at(key) = std::stoi(val);
    else if (key == "w00") c.w00 = std::stod(val);
    else if (key == "g_ord1") c.g_ord1 = std::stod(val);
    else if (key == "lds32") c.lds32 = (size_t)std::stoul(val);
    else return false;
    return true;
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream words(line);
        std::string name, word;
        if (!(words >> name)) continue;
        MergeCall c;
        std::vector<std::string> env;
        while (words >> word) {
            const size_t eq = word.find('=');
            if (eq == std::string::npos) { fprintf(stderr, "%s: no '=' in %s\n", name.c_str(), word.c_str()); return 2; }
            const std::string key = word.substr(0, eq), val = word.substr(eq + 1);
            if (key.rfind("ANSFM_", 0) == 0) { setenv(key.c_str(), val.c_str(), 1); env.push_back(key); }
            else if (!set_field(c, key, val)) { fprintf(stderr, "%s: unknown field %s\n", name.c_str(), key.c_str()); return 2; }
        }
        const MergePlan m = merge_plan(c, merge_switches_from_env());
        for (const std::string &key : env) unsetenv(key.c_str());
        const int list = by_list_len(c.G, [](auto d) { return (int)decltype(d)::value; });
        printf("%s sorted=%d nodiv=%d nobox=%d keys32=%d opt=%d lane_rows=%d lane_nv=%d rowmajor=%d gfast=%d nwaves=%d lds=%zu "
               "grid=%ld scratch=%zu flags=%d trims=%d width=%d list=%d\n",
               name.c_str(), (int)m.sorted, (int)m.nodiv, (int)m.nobox, (int)m.keys32, m.opt, (int)m.lane_rows, m.lane_nv,
               (int)m.rowmajor, (int)m.gfast, m.nwaves, m.lds, m.grid, m.scratch_bytes_per_block, m.flags, m.trims, m.group_width,
               list);
    }
    return 0;
}

// Prints the decisions of bevgen_amd/csrc/vq_plan.h (the pure part of the VQGAN host driver) for the cases it is given - host code only, no HIP header, no GPU.
// tests/test_vq_plan_cpu.py builds it (with the address and undefined-behaviour sanitizers) and compares its output with the expected values.
//
// One case per line of stdin: a function name, then blank-separated key=value tokens.  Integers, except the per-level lists (comma-separated, level 0 first).
//   shape, every function but `cut`: encoder levels ch ch_mult=.. attn=.. nin=.. first_nin=.. resample=.. mid_nin cin_pad
//   scan   h w          -> vq_scan (decoder: the latent grid, encoder: the image)
//   cut    n            -> vq_pass_cut, and the images of every pass
//   sites               -> vq_sites_per_pass, vq_feeds_nin per level
//   up     C planes range sw.up_planes   -> vq_up_form (0 planes, 1 ranged fp32, 2 plain)
// One JSON object per case.
#include "vq_plan.h"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

using namespace bevgen;

static void run_case(const std::string& line) {
    std::istringstream in(line);
    std::string fn, tok;
    if (!(in >> fn)) return;
    std::map<std::string, std::string> kv;
    static const char* known[] = {"encoder", "levels", "ch", "ch_mult", "attn", "nin", "first_nin", "resample", "mid_nin", "cin_pad", "h", "w", "n", "C", "planes", "range", "sw.up_planes"};
    while (in >> tok) {
        const size_t eq = tok.find('=');
        bool ok = false;
        if (eq != std::string::npos)
            for (const char* k : known) ok = ok || tok.substr(0, eq) == k;
        if (!ok) {
            std::printf("{\"error\": \"bad token %s\"}\n", tok.c_str());
            return;
        }
        kv[tok.substr(0, eq)] = tok.substr(eq + 1);
    }
    const auto get = [&](const char* k, long dflt) { const auto it = kv.find(k); return it == kv.end() ? dflt : std::atol(it->second.c_str()); };
    // a per-level list into at most kVqMaxLevels entries; false: too many
    const auto list = [&](const char* k, auto* out) {
        const auto it = kv.find(k);
        if (it == kv.end()) return true;
        std::istringstream ls(it->second);
        std::string item;
        int i = 0;
        while (std::getline(ls, item, ',')) {
            if (i == kVqMaxLevels) return false;
            out[i++] = std::atoi(item.c_str());
        }
        return true;
    };

    VqShape sh;
    sh.encoder = get("encoder", 0) != 0;
    sh.levels = (int)get("levels", 0); sh.ch = (int)get("ch", 0); sh.mid_nin = (int)get("mid_nin", 0); sh.cin_pad = (int)get("cin_pad", 0);
    if (sh.levels < 0 || sh.levels > kVqMaxLevels || !list("ch_mult", sh.ch_mult) || !list("attn", sh.attn) || !list("nin", sh.nin) || !list("first_nin", sh.first_nin) ||
        !list("resample", sh.resample)) {
        std::printf("{\"error\": \"more than %d levels\"}\n", kVqMaxLevels);
        return;
    }

    if (fn == "scan") {
        if (sh.levels < 1) { std::printf("{\"error\": \"scan needs a shape\"}\n"); return; }
        const VqSizes z = vq_scan(sh, (int)get("h", 0), (int)get("w", 0));
        std::printf("{\"per_img\": %ld, \"max_c\": %d, \"attn_hw\": %ld, \"attn_hwp\": %ld, \"lat\": [%d, %d], \"image\": [%d, %d]}\n", z.per_img, z.max_c, z.attn_hw, z.attn_hwp, z.lat_h,
                    z.lat_w, z.RH, z.RW);
    } else if (fn == "cut") {
        const int n = (int)get("n", 0);
        const VqPasses p = vq_pass_cut(n);
        std::printf("{\"chunk\": %d, \"passes\": %d, \"images\": [", p.chunk, p.passes);
        for (int i = 0; i < p.passes; ++i) std::printf("%s%d", i ? ", " : "", std::min(p.chunk, n - i * p.chunk));
        std::printf("]}\n");
    } else if (fn == "sites") {
        std::printf("{\"per_pass\": %d, \"feeds_nin\": [", vq_sites_per_pass(sh));
        for (int l = 0; l < sh.levels; ++l) std::printf("%s%d", l ? ", " : "", (int)vq_feeds_nin(sh, l));
        std::printf("]}\n");
    } else if (fn == "up") {
        VqSwitches sw;
        sw.up_planes = get("sw.up_planes", 1) != 0;
        std::printf("{\"form\": %d}\n", (int)vq_up_form((int)get("C", 0), get("planes", 0) != 0, get("range", 0) != 0, sw));
    } else {
        std::printf("{\"error\": \"bad function %s\"}\n", fn.c_str());
    }
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) run_case(line);
    return 0;
}

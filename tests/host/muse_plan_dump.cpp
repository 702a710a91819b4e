// Prints the decisions of bevgen_amd/csrc/muse_plan.h (how a Route M forward launches its projections) for the cases it is given - host code only, no HIP call, no GPU.
// tests/test_muse_plan_cpu.py builds it (with the address and undefined-behaviour sanitizers) and compares its output with the expected decisions.
//
// One case per line of stdin: a function name, then blank-separated key=value tokens (integers).
//   ksplit  rows N K                                  -> pick_ksplit
//   attn    blocks tiles                              -> pick_attn_ksplit
//   kpart   rows D Fpad                               -> muse_needs_kpart
//   rules   rows consts (fold constants exist)        -> muse_fold_level, muse_tile_merge, muse_qkv_merged
//   proj    kind (MuseProj) M N K fold merged kpart sk_ws   -> muse_proj_plan
//   switches, any function: sw.<field of MuseSwitches>, gsw.sk (GldsSwitches::sk, $BEVGEN_GEMM_SK)
// One JSON object per case.
#include "muse_plan.h"

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
    std::map<std::string, long> kv;
    static const char* known[] = {"rows", "N", "K", "M", "D", "Fpad", "blocks", "tiles", "consts", "kind", "fold", "merged", "kpart", "sk_ws", "sw.ln_fold", "sw.ln_merge",
                                  "sw.qkv_merge", "sw.qkv_wm4", "sw.ksplit", "sw.attn_ksplit", "gsw.sk"};
    while (in >> tok) {
        const size_t eq = tok.find('=');
        bool ok = false;
        if (eq != std::string::npos)
            for (const char* k : known) ok = ok || tok.substr(0, eq) == k;
        if (!ok) {
            std::printf("{\"error\": \"bad token %s\"}\n", tok.c_str());
            return;
        }
        kv[tok.substr(0, eq)] = std::atol(tok.c_str() + eq + 1);
    }
    const auto get = [&](const char* k, long dflt) { const auto it = kv.find(k); return it == kv.end() ? dflt : it->second; };

    MuseSwitches sw;
    const struct { const char* name; int* field; } fields[] = {{"sw.ln_fold", &sw.ln_fold},   {"sw.ln_merge", &sw.ln_merge}, {"sw.qkv_merge", &sw.qkv_merge},
                                                               {"sw.qkv_wm4", &sw.qkv_wm4},   {"sw.ksplit", &sw.ksplit},     {"sw.attn_ksplit", &sw.attn_ksplit}};
    for (const auto& f : fields) *f.field = (int)get(f.name, *f.field);
    GldsSwitches gsw;
    gsw.sk = (int)get("gsw.sk", gsw.sk);

    if (fn == "ksplit") {
        std::printf("{\"ksplit\": %d}\n", pick_ksplit(get("rows", 0), (int)get("N", 0), (int)get("K", 0), sw.ksplit));
    } else if (fn == "attn") {
        std::printf("{\"attn_ksplit\": %d}\n", pick_attn_ksplit(get("blocks", 0), (int)get("tiles", 0), sw.attn_ksplit));
    } else if (fn == "kpart") {
        std::printf("{\"kpart\": %d}\n", (int)muse_needs_kpart(get("rows", 0), (int)get("D", 0), (int)get("Fpad", 0), sw));
    } else if (fn == "rules") {
        const long rows = get("rows", 0);
        std::printf("{\"fold\": %d, \"tile_merge\": %d, \"qkv_merged\": %d}\n", muse_fold_level(sw, get("consts", 1) != 0), (int)muse_tile_merge(sw, rows),
                    (int)muse_qkv_merged(sw, rows));
    } else if (fn == "proj") {
        MuseProjIn p;
        p.kind = (MuseProj)get("kind", PROJ_UP);
        p.M = get("M", 0); p.N = (int)get("N", 0); p.K = (int)get("K", 0);
        p.fold_role = get("fold", 0) != 0; p.merged = get("merged", 0) != 0;
        p.has_kpart = get("kpart", 0) != 0; p.has_sk_ws = get("sk_ws", 0) != 0;
        const MuseProjPlan r = muse_proj_plan(p, sw, gsw);
        std::printf("{\"sk_asked\": %d, \"sk\": %d, \"kpart\": %d, \"ksplit\": %d, \"q_unfused\": %d, \"force_wm\": %d}\n", (int)r.sk_asked, (int)r.sk, (int)r.kpart, r.ksplit,
                    (int)r.q_unfused, r.force_wm);
    } else {
        std::printf("{\"error\": \"bad function %s\"}\n", fn.c_str());
    }
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) run_case(line);
    return 0;
}

// Prints the decisions of bevgen_amd/csrc/ar_plan.h (the shape of a Route A decode step) for the cases it is given - host code only, no HIP call, no GPU.
// tests/test_ar_plan_cpu.py builds it (with the address and undefined-behaviour sanitizers) and compares its output with the expected decisions.
//
// One case per line of stdin: a function name, then blank-separated key=value tokens (integers).
//   ksplit  N K                       -> skinny_fused_ksplit
//   splits  B H L                     -> decode_attention_splits
//   lds     G D L                     -> ar_attn_fused_lds_bytes (L rounded up to 4, as the plan asks)
//   graph   steps logits prof off     -> ar_use_graph
//   plan    B G + model + context     -> ar_step_plan at (B, G)
//   prefill B S + model + context     -> ar_prefill_group (the G that ar_prefill asks with) and ar_step_plan at (B, that G)
//   model: D H K L V (default: config 4 - 1024, 16, 256, 2368, 1024); context: path (BEVGEN_DECODE_*, default auto) wf16 chains trace ready cus placement
//   (mlpf_device_ok = mlp_fused_cus_ok(cus, D) && placement; default 256 CUs, verified, ready); switches: sw.ln2_fold sw.pick_tail sw.mlp_fuse
// One JSON object per case.
#include "ar_plan.h"

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
    static const char* known[] = {"B", "G", "S", "D", "H", "K", "L", "V", "N", "path", "wf16", "chains", "trace", "ready", "cus", "placement", "steps", "logits", "prof", "off",
                                  "sw.ln2_fold", "sw.pick_tail", "sw.mlp_fuse"};
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

    ArSwitches sw;
    sw.ln2_fold = (int)get("sw.ln2_fold", sw.ln2_fold); sw.pick_tail = (int)get("sw.pick_tail", sw.pick_tail); sw.mlp_fuse = (int)get("sw.mlp_fuse", sw.mlp_fuse);
    ArPlanIn p;
    p.B = (int)get("B", 1); p.G = (int)get("G", 1);
    p.D = (int)get("D", 1024); p.H = (int)get("H", 16); p.K = (int)get("K", 256); p.L = (int)get("L", 2368); p.V = (int)get("V", 1024);
    p.decode_path = (int)get("path", BEVGEN_DECODE_AUTO); p.w_f16 = get("wf16", 0) != 0; p.chains = (int)get("chains", 0); p.trace = get("trace", 0) != 0;
    p.mlpf_ready = get("ready", 1) != 0;
    p.mlpf_device_ok = mlp_fused_cus_ok((int)get("cus", 256), p.D) && get("placement", 1) != 0;

    if (fn == "ksplit") {
        std::printf("{\"ksplit\": %d}\n", skinny_fused_ksplit((int)get("N", 0), (int)get("K", 0)));
    } else if (fn == "splits") {
        std::printf("{\"splits\": %d}\n", decode_attention_splits(p.B, p.H, p.L));
    } else if (fn == "lds") {
        std::printf("{\"lds\": %zu}\n", ar_attn_fused_lds_bytes(p.G, p.D, (int)round_up(p.L, 4)));
    } else if (fn == "graph") {
        std::printf("{\"graph\": %d}\n", (int)ar_use_graph((int)get("steps", 0), get("logits", 0) != 0, get("prof", 0) != 0, get("off", 0) != 0));
    } else if (fn == "plan" || fn == "prefill") {
        if (fn == "prefill") p.G = ar_prefill_group(p, sw, (int)get("S", 1));
        const ArStepPlan r = ar_step_plan(p, sw);
        std::printf("{\"G\": %d, \"path\": %d, \"fused\": %d, \"split\": %d, \"chains\": %d, \"Bc\": %d, \"mlp_fused\": %d, \"ln2_fold\": %d, \"down_ksplit\": %d, \"attn_ksplit\": %d, "
                    "\"pick_embeds\": %d, \"needs_split_qkv_image\": %d}\n",
                    p.G, r.path, (int)r.fused, (int)r.split, r.chains, r.Bc, (int)r.mlp_fused, (int)r.ln2_fold, r.down_ksplit, r.attn_ksplit, (int)r.pick_embeds,
                    (int)r.needs_split_qkv_image);
    } else {
        std::printf("{\"error\": \"bad function %s\"}\n", fn.c_str());
    }
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) run_case(line);
    return 0;
}

// Prints the launch plan of the LDS-DMA GEMM (bevgen_amd/csrc/gemm_plan.h) for the cases it is given - host code only, no HIP call, no GPU.
// tests/test_gemm_plan_cpu.py builds it (with the address and undefined-behaviour sanitizers) and compares its output with the expected plans.
//
// One case per line of stdin (or per argument): blank-separated key=value tokens.
//   problem   M N K ksplit w16 epi act batch lda ldb ldc ldr m_base force_wm no_row_split   (lda / ldb default to K, ldc / ldr to N)
//   pointers  R bias_n bias_m kpart gn_part sk_ws ln_in_stats ln_in_gsums ln_in_cs ln_out   (1 = a 16-byte-aligned dummy, 2 = a misaligned one; never dereferenced)
//             A_hi (default 1; 0 = operands not pre-split)     epi != 0 sets every epilogue pointer, epi_rows (default M), epi_heads (default from N), epi_ld
//   conv      conv=1 n h w cin up stride pad hin win general   (M = n h w output pixels, K = 9 cin unless K is given)
//   LayerNorm ln_rows ln_in_groups ln_in_count ln_out_ld
//   stream-K  sk_force cus (default 256) xcd (the placement probe's answer, default 1)
//   switches  sw.<field of GldsSwitches>
// One line of output per case: a JSON object with the launches (or the refusal's text) and how often the placement probe was asked.
#include "gemm_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

using namespace bevgen;

static int g_xcd_calls = 0;
static bool g_xcd_answer = true;
static bool xcd_probe() {
    ++g_xcd_calls;
    return g_xcd_answer;
}

alignas(64) static char g_dummy[64];
template <class T>
static T* dummy(long kind) { return kind == 0 ? nullptr : reinterpret_cast<T*>(g_dummy + (kind == 2 ? 4 : 0)); }

static void run_case(const std::string& line) {
    std::map<std::string, long> kv;
    std::istringstream in(line);
    std::string tok;
    while (in >> tok) {
        const size_t eq = tok.find('=');
        if (eq == std::string::npos) {
            std::printf("{\"error\": \"bad token %s\"}\n", tok.c_str());
            return;
        }
        kv[tok.substr(0, eq)] = std::atol(tok.c_str() + eq + 1);
    }
    if (kv.empty()) return;
    const auto get = [&](const char* k, long dflt) { const auto it = kv.find(k); return it == kv.end() ? dflt : it->second; };

    GemmArgs g;
    if (get("conv", 0)) {
        g.mode = MODE_CONV3;
        g.conv_h = (int)get("h", 0);
        g.conv_w = (int)get("w", 0);
        g.conv_cin = (int)get("cin", 0);
        g.conv_up = (int)get("up", 0);
        g.conv_stride = (int)get("stride", 0);
        g.conv_pad = (int)get("pad", -1);
        g.conv_hin = (int)get("hin", 0);
        g.conv_win = (int)get("win", 0);
        g.conv_general = get("general", 0) != 0;
        g.M = (int)(get("n", 1) * g.conv_h * g.conv_w);
        g.K = (int)get("K", 9 * g.conv_cin);
    } else {
        g.K = (int)get("K", 0);
    }
    g.M = (int)get("M", g.M);
    g.N = (int)get("N", 0);
    g.lda = (int)get("lda", g.K);
    g.ldb = (int)get("ldb", g.K);
    g.ldc = (int)get("ldc", g.N);
    g.ldr = (int)get("ldr", g.N);
    g.batch = (int)get("batch", 1);
    g.act = (int)get("act", ACT_NONE);
    g.ksplit = (int)get("ksplit", 1);
    g.m_base = (int)get("m_base", 0);
    g.force_wm = (int)get("force_wm", 0);
    g.no_row_split = get("no_row_split", 0) != 0;
    g.b_lo_zero = get("w16", 0) != 0;
    g.C = dummy<float>(get("C", 1));
    g.R = dummy<const float>(get("R", 0));
    g.bias_n = dummy<const float>(get("bias_n", 0));
    g.bias_m = dummy<const float>(get("bias_m", 0));
    g.kpart = dummy<float>(get("kpart", 0));
    g.gn_part = dummy<float>(get("gn_part", 0));
    g.sk_ws = dummy<void>(get("sk_ws", 0));
    g.sk_force = get("sk_force", 0) != 0;
    g.A_hi = g.B_hi = dummy<const uint16_t>(get("A_hi", 1));
    g.A_lo = g.B_lo = g.A_hi;
    g.epi = (int)get("epi", 0);
    if (g.epi != 0) {
        g.epi_scale = g.epi_qscale = dummy<const float>(1);
        g.epi_hi = g.epi_lo = g.epi_hi2 = g.epi_lo2 = g.epi_qh = g.epi_ql = dummy<void>(1);
        g.epi_aux = dummy<const void>(1);
        g.epi_rows = (int)get("epi_rows", g.M);
        g.epi_heads = (int)get("epi_heads", g.N / 64 / (g.epi == EPI_MUSE_QKV ? 3 : g.epi == EPI_MUSE_KV ? 2 : 1));
        g.epi_ld = (int)get("epi_ld", g.epi_rows + 1);
    }
    g.ln_in_stats = dummy<const float>(get("ln_in_stats", 0));
    g.ln_in_gsums = dummy<const float>(get("ln_in_gsums", 0));
    g.ln_in_cs = dummy<const float>(get("ln_in_cs", (g.ln_in_stats || g.ln_in_gsums) ? 1 : 0));
    g.ln_in_groups = (int)get("ln_in_groups", g.K / 32);
    g.ln_in_count = (int)get("ln_in_count", g.K);
    g.ln_rows = (int)get("ln_rows", g.M);
    g.ln_out_planes = dummy<void>(get("ln_out", 0));
    g.ln_out_stats = dummy<float>(get("ln_out", 0));
    g.ln_out_ld = (int)get("ln_out_ld", g.N);

    GldsSwitches sw;
    const struct { const char* name; int* field; } fields[] = {
        {"sw.sk", &sw.sk}, {"sw.rpf", &sw.rpf}, {"sw.rme", &sw.rme}, {"sw.band", &sw.band}, {"sw.wm", &sw.wm}, {"sw.top_wm", &sw.top_wm},
        {"sw.rowsplit", &sw.rowsplit}, {"sw.bot_wm", &sw.bot_wm}, {"sw.stages", &sw.stages}, {"sw.conv_thin", &sw.conv_thin}, {"sw.half8", &sw.half8},
        {"sw.conv_fast", &sw.conv_fast}};
    for (const auto& f : fields) *f.field = (int)get(f.name, *f.field);

    g_xcd_calls = 0;
    g_xcd_answer = get("xcd", 1) != 0;
    try {
        const GldsPlan p = plan_gemm_split_glds(g, sw, (int)get("cus", 256), &xcd_probe);
        std::printf("{\"launches\": [");
        for (int i = 0; i < p.n; ++i) {
            const GldsLaunch& l = p.l[i];
            const int idx = glds_variant_index(l.v);
            std::printf("%s{\"rows\": [%d, %d], \"variant\": [%d, %d, %d, %d, %d, %d], \"w16\": %d, \"sk\": %d, \"grid\": [%u, %u, %u], \"threads\": %d, \"lds\": %zu, "
                        "\"prof\": \"%s\", \"reduce\": %d, \"in_table\": %d, \"lds_max\": %zu, \"tile_band\": %d, \"r_prefetch\": %d, \"row_major_epi\": %d, "
                        "\"force_wm\": %d, \"no_row_split\": %d, \"sk_tiles\": %d, \"a_bytes\": %d, \"work\": %.17g}",
                        i ? ", " : "", l.g.m_base, l.g.M, l.v.mode, l.v.wm, l.v.s, (int)l.v.ks, l.v.ti, l.v.tj, (int)l.v.w16, (int)l.v.sk, l.grid.x, l.grid.y, l.grid.z, l.threads,
                        l.lds, l.prof_kind == PROF_GEMM ? "G" : l.prof_kind == PROF_GEMM_SMALL ? "S" : l.prof_kind == PROF_CONV3 ? "C" : "?", (int)l.reduce_after, (int)(idx >= 0),
                        idx >= 0 ? glds_lds_max(kGldsVariants[idx]) : (size_t)0, l.g.tile_band, (int)l.g.r_prefetch, (int)l.g.row_major_epi, l.g.force_wm, (int)l.g.no_row_split,
                        l.g.sk_tiles, l.g.a_bytes, l.work);
        }
        std::printf("], \"xcd_calls\": %d}\n", g_xcd_calls);
    } catch (const Error& e) {
        std::string msg;
        for (const char* c = e.what(); *c; ++c) {
            if (*c == '"' || *c == '\\') msg += '\\';
            msg += *c;
        }
        std::printf("{\"error\": \"%s\", \"xcd_calls\": %d}\n", msg.c_str(), g_xcd_calls);
    }
}

int main(int argc, char** argv) {
    if (argc > 1) {
        for (int i = 1; i < argc; ++i) run_case(argv[i]);
    } else {
        std::string line;
        while (std::getline(std::cin, line)) run_case(line);
    }
    // the table itself: one line, so that the test can check its size and that no tuple is listed twice
    std::printf("{\"table\": [");
    for (int i = 0; i < kGldsVariantCount; ++i) {
        const GldsVariant& v = kGldsVariants[i];
        std::printf("%s[%d, %d, %d, %d, %d, %d, %d, %d]", i ? ", " : "", v.mode, v.wm, v.s, (int)v.w16, (int)v.ks, v.ti, v.tj, (int)v.sk);
    }
    std::printf("]}\n");
    return 0;
}

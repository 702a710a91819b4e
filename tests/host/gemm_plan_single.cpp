// Launch plan of the LDS-DMA GEMM (bevgen_amd/csrc/gemm_plan.h) for a single-product launch (GemmArgs::a_hi_only) - host code only, no HIP call, no GPU.
// tests/test_single_product_cpu.py builds it (with the address and undefined-behaviour sanitizers) and checks its output.
//
// One case per line of stdin: blank-separated key=value tokens, the subset of tests/host/gemm_plan_dump.cpp's that tests/test_gemm_plan_cpu.py's EXPECTED table uses
//   M N K R epi epi_rows force_wm ksplit kpart ln_in_gsums   |   conv=1 n h w cin up          (weights are f16-representable: b_lo_zero is set)
// One JSON object per case:
//   same       the plan with a_hi_only equals the plan without it field for field (default switches, no stream-K workspace)
//   launches   its number of launches
//   sk_plain   with a stream-K workspace, the switch at 2 and the per-call force: how many launches of the plan WITHOUT the flag take the stream-K form
//   sk_single  the same count WITH the flag (must be 0), and
//   sk_same    that plan equals the default-switch plan but for the workspace pointer
#include "gemm_plan.h"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

using namespace bevgen;

static bool xcd_probe() { return true; }
alignas(64) static char g_dummy[64];
template <class T>
static T* dummy(long on) { return on ? reinterpret_cast<T*>(g_dummy) : nullptr; }

static bool same_launch(const GldsLaunch& a, const GldsLaunch& b) {
    const GemmArgs &x = a.g, &y = b.g;
    return a.v.mode == b.v.mode && a.v.wm == b.v.wm && a.v.s == b.v.s && a.v.w16 == b.v.w16 && a.v.ks == b.v.ks && a.v.ti == b.v.ti && a.v.tj == b.v.tj && a.v.sk == b.v.sk &&
           a.grid.x == b.grid.x && a.grid.y == b.grid.y && a.grid.z == b.grid.z && a.threads == b.threads && a.lds == b.lds && a.prof_kind == b.prof_kind && a.work == b.work &&
           a.reduce_after == b.reduce_after && x.M == y.M && x.m_base == y.m_base && x.N == y.N && x.K == y.K && x.ksplit == y.ksplit && x.tile_band == y.tile_band &&
           x.force_wm == y.force_wm && x.no_row_split == y.no_row_split && x.row_major_epi == y.row_major_epi && x.r_prefetch == y.r_prefetch && x.sk_tiles == y.sk_tiles &&
           x.a_bytes == y.a_bytes && x.b_lo_zero == y.b_lo_zero && x.conv_stride == y.conv_stride && x.conv_pad == y.conv_pad && x.conv_hin == y.conv_hin && x.conv_win == y.conv_win;
}
static bool same_plan(const GldsPlan& a, const GldsPlan& b) {
    if (a.n != b.n) return false;
    for (int i = 0; i < a.n; ++i)
        if (!same_launch(a.l[i], b.l[i])) return false;
    return true;
}
static int sk_launches(const GldsPlan& p) {
    int n = 0;
    for (int i = 0; i < p.n; ++i) n += p.l[i].v.sk ? 1 : 0;
    return n;
}

static void run_case(const std::string& line) {
    std::map<std::string, long> kv;
    std::istringstream in(line);
    std::string tok;
    static const char* known[] = {"M", "N", "K", "R", "epi", "epi_rows", "force_wm", "ksplit", "kpart", "ln_in_gsums", "conv", "n", "h", "w", "cin", "up"};
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
    if (kv.empty()) return;
    const auto get = [&](const char* k, long dflt) { const auto it = kv.find(k); return it == kv.end() ? dflt : it->second; };

    GemmArgs g;
    if (get("conv", 0)) {
        g.mode = MODE_CONV3;
        g.conv_h = (int)get("h", 0);
        g.conv_w = (int)get("w", 0);
        g.conv_cin = (int)get("cin", 0);
        g.conv_up = (int)get("up", 0);
        g.M = (int)(get("n", 1) * g.conv_h * g.conv_w);
        g.K = 9 * g.conv_cin;
    } else {
        g.M = (int)get("M", 0);
        g.K = (int)get("K", 0);
    }
    g.N = (int)get("N", 0);
    g.lda = g.ldb = g.K;
    g.ldc = g.ldr = g.N;
    g.ksplit = (int)get("ksplit", 1);
    g.force_wm = (int)get("force_wm", 0);
    g.b_lo_zero = true;
    g.C = dummy<float>(1);
    g.R = dummy<const float>(get("R", 0));
    g.kpart = dummy<float>(get("kpart", 0));
    g.A_hi = g.A_lo = g.B_hi = g.B_lo = dummy<const uint16_t>(1);
    g.epi = (int)get("epi", 0);
    if (g.epi != 0) {
        g.epi_scale = g.epi_qscale = dummy<const float>(1);
        g.epi_hi = g.epi_lo = g.epi_hi2 = g.epi_lo2 = g.epi_qh = g.epi_ql = dummy<void>(1);
        g.epi_aux = dummy<const void>(1);
        g.epi_rows = (int)get("epi_rows", g.M);
        g.epi_heads = g.N / 64 / (g.epi == EPI_MUSE_QKV ? 3 : g.epi == EPI_MUSE_KV ? 2 : 1);
        g.epi_ld = g.epi_rows + 1;
    }
    g.ln_in_gsums = dummy<const float>(get("ln_in_gsums", 0));
    g.ln_in_cs = dummy<const float>(g.ln_in_gsums ? 1 : 0);
    g.ln_in_groups = g.K / 32;
    g.ln_in_count = g.K;
    g.ln_rows = g.M;

    try {
        GemmArgs gs = g;
        gs.a_hi_only = true;
        const GldsSwitches dflt;
        const GldsPlan plain = plan_gemm_split_glds(g, dflt, 256, &xcd_probe), single = plan_gemm_split_glds(gs, dflt, 256, &xcd_probe);
        GldsSwitches sk;
        sk.sk = 2;
        GemmArgs gk = g, gks = gs;
        gk.sk_ws = gks.sk_ws = dummy<void>(1);
        gk.sk_force = gks.sk_force = true;
        const GldsPlan plain_sk = plan_gemm_split_glds(gk, sk, 256, &xcd_probe), single_sk = plan_gemm_split_glds(gks, sk, 256, &xcd_probe);
        std::printf("{\"same\": %d, \"launches\": %d, \"sk_plain\": %d, \"sk_single\": %d, \"sk_same\": %d}\n", (int)same_plan(plain, single), single.n, sk_launches(plain_sk),
                    sk_launches(single_sk), (int)same_plan(plain, single_sk));
    } catch (const Error& e) {
        std::printf("{\"error\": \"refused\"}\n");
    }
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) run_case(line);
    return 0;
}

// bevgen_amd/csrc/ar_plan.h with int8 decode weights (ArPlanIn::w_f16 = 2) against fp16 ones (= 1) over a grid of inputs - host code only, no HIP call, no GPU.
// tests/test_decode_w_i8_cpu.py builds it (with the address and undefined-behaviour sanitizers) and reads its one JSON line: the number of inputs compared, the number
// at which any decision differs (expected: none - the int8 image keeps the fp16 image's lane map and shape rules), and, as a check that the grid can tell storage kinds
// apart at all, the number at which the fp32 plan differs from the fp16 one.
#include "ar_plan.h"

#include <cstdio>
#include <type_traits>

using namespace bevgen;

static_assert(std::is_same<decltype(ArPlanIn::w_f16), int>::value, "ArPlanIn::w_f16 is the storage kind (0 fp32, 1 fp16, 2 int8), not a flag");

static bool same(const ArStepPlan& a, const ArStepPlan& b) {
    return a.path == b.path && a.fused == b.fused && a.split == b.split && a.chains == b.chains && a.Bc == b.Bc && a.mlp_fused == b.mlp_fused && a.ln2_fold == b.ln2_fold &&
           a.down_ksplit == b.down_ksplit && a.attn_ksplit == b.attn_ksplit && a.pick_embeds == b.pick_embeds && a.needs_split_qkv_image == b.needs_split_qkv_image;
}

int main() {
    long cases = 0, differ = 0, f32_differs = 0;
    const int paths[] = {BEVGEN_DECODE_FUSED, BEVGEN_DECODE_PER_OP, BEVGEN_DECODE_SPLIT, BEVGEN_DECODE_AUTO};
    const int dims[][2] = {{1024, 16}, {256, 4}, {512, 8}, {128, 2}, {768, 12}};   // (D, H): config 4, the test presets, widths the 2-byte / 1-byte images refuse
    const int batches[] = {1, 2, 3, 4, 5, 8, 16, 33, 64, 65};
    for (int path : paths)
        for (const auto& dh : dims)
            for (int B : batches)
                for (int G : {1, 2, 4})
                    for (int ready = 0; ready < 2; ++ready)
                        for (int dev_ok = 0; dev_ok < 2; ++dev_ok)
                            for (int fuse = 0; fuse < 2; ++fuse)
                                for (int chains : {0, 2})
                                    for (int V : {1024, 64, 1000}) {
                                        if (B % G) continue;
                                        ArSwitches sw;
                                        sw.mlp_fuse = fuse;
                                        ArPlanIn in;
                                        in.B = B; in.G = G; in.D = dh[0]; in.H = dh[1]; in.K = 256; in.L = 2368; in.V = V;
                                        in.decode_path = path; in.chains = chains; in.mlpf_ready = ready != 0; in.mlpf_device_ok = dev_ok != 0;
                                        ArPlanIn f32 = in, f16 = in, i8 = in;
                                        f32.w_f16 = 0; f16.w_f16 = 1; i8.w_f16 = 2;
                                        ++cases;
                                        const bool eq = same(ar_step_plan(f16, sw), ar_step_plan(i8, sw)) && ar_prefill_group(f16, sw, G) == ar_prefill_group(i8, sw, G) &&
                                                        ar_split_supported(f16) == ar_split_supported(i8) && ar_fused(f16, sw) == ar_fused(i8, sw);
                                        if (!eq) ++differ;
                                        if (!same(ar_step_plan(f32, sw), ar_step_plan(f16, sw))) ++f32_differs;
                                    }
    // config 4, decode_path = auto, one sequence: the fused layer (as with fp16 weights), where fp32 weights take the split one
    ArPlanIn one;
    one.B = 1; one.D = 1024; one.H = 16; one.K = 256; one.L = 2368; one.V = 1024; one.decode_path = BEVGEN_DECODE_AUTO; one.mlpf_ready = true; one.mlpf_device_ok = true;
    ArSwitches sw;
    one.w_f16 = 2;
    const ArStepPlan p8 = ar_step_plan(one, sw);
    one.w_f16 = 0;
    const ArStepPlan p32 = ar_step_plan(one, sw);
    std::printf("{\"cases\": %ld, \"differ\": %ld, \"f32_differs\": %ld, \"i8_auto_b1\": [%d, %d, %d], \"f32_auto_b1\": [%d, %d, %d]}\n", cases, differ, f32_differs, p8.path,
                (int)p8.fused, (int)p8.mlp_fused, p32.path, (int)p32.fused, (int)p32.mlp_fused);
    return 0;
}

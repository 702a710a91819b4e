// Host-only check of the workspace arena (bevgen_amd/csrc/arena.h): metering against real carving over pseudo-random allocation sequences, and the carve() helper.
// Built without any HIP header, with the address and undefined-behaviour sanitizers, by tests/test_arena_cpu.py; reserve / release are malloc-backed here.
// Prints one JSON line per check; the exit status is the number of failed checks.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "arena.h"

namespace bevgen {
static int g_reserves = 0, g_mallocs = 0;
static size_t g_last_reserve = 0;
void Arena::reserve(size_t bytes) {   // the library's rule (context.cpp) over malloc
    ++g_reserves;
    g_last_reserve = bytes;
    if (bytes <= cap) return;
    free(base);
    base = static_cast<char*>(aligned_alloc(256, (bytes + 255) & ~size_t(255)));
    ++g_mallocs;
    cap = bytes;
    off = 0;
}
void Arena::release() {
    free(base);
    base = nullptr;
    cap = off = 0;
}
}  // namespace bevgen

using bevgen::Arena;

static unsigned long long g_rng = 0x9E3779B97F4A7C15ull;
static unsigned long long rnd() {   // xorshift64*
    g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27;
    return g_rng * 0x2545F4914F6CDD1Dull;
}
static size_t rnd_size() {
    switch (rnd() % 6) {
        case 0: return 0;
        case 1: return 1;
        case 2: return rnd() % 512;               // around the alignment
        case 3: return 256 * (rnd() % 64);        // exact multiples of it
        case 4: return rnd() % (64 * 1024);
        default: return rnd() % (6 * 1024 * 1024);   // several MB
    }
}

static int g_failed = 0;
static void report(const char* name, bool ok, const char* detail = "") {
    printf("{\"check\": \"%s\", \"ok\": %s, \"detail\": \"%s\"}\n", name, ok ? "true" : "false", detail);
    if (!ok) ++g_failed;
}

static bool exhausted(Arena& a, const std::vector<size_t>& sizes) {   // does carving `sizes` from a (reset) raise the arena's exhaustion error?
    a.reset();
    try {
        for (size_t b : sizes) (void)a.alloc(b);
    } catch (const bevgen::Error& e) {
        return e.code == -4 && strstr(e.what(), "workspace arena exhausted") != nullptr;
    }
    return false;
}

int main() {
    const int kSequences = 300;
    bool same_offsets = true, aligned = true, total_equal = true, nonnull = true, one_less_fails = true, exact_fits = true;
    int allocs = 0;
    for (int it = 0; it < kSequences; ++it) {
        std::vector<size_t> sizes(1 + rnd() % 24);
        for (size_t& b : sizes) b = rnd_size();
        if (it == 0) sizes.assign({0});            // the degenerate sequences
        if (it == 1) sizes.assign({1});
        if (it == 2) sizes.assign({0, 0, 1, 0});
        Arena m;
        m.metering = true;
        m.base = reinterpret_cast<char*>(uintptr_t(256));
        std::vector<size_t> moff;
        for (size_t b : sizes) {
            char* p = static_cast<char*>(m.alloc(b));
            nonnull = nonnull && p != nullptr;
            moff.push_back((size_t)(p - m.base));
        }
        const size_t total = m.off;
        Arena r;
        r.reserve(total);
        for (size_t i = 0; i < sizes.size(); ++i) {
            char* p = static_cast<char*>(r.alloc(sizes[i]));
            const size_t o = (size_t)(p - r.base);
            same_offsets = same_offsets && o == moff[i];
            aligned = aligned && o % 256 == 0 && moff[i] % 256 == 0 && reinterpret_cast<uintptr_t>(p) % 256 == 0;
            if (sizes[i]) memset(p, 0xA5, sizes[i]);   // (the sanitizer sees every byte the layout hands out)
            ++allocs;
        }
        total_equal = total_equal && r.off == total;
        exact_fits = exact_fits && !exhausted(r, sizes);
        if (total > 0) {
            r.cap = total - 1;   // the same slab, one byte short
            one_less_fails = one_less_fails && exhausted(r, sizes);
            r.cap = total;
        }
        r.release();
    }
    char detail[96];
    snprintf(detail, sizeof detail, "%d sequences, %d allocations", kSequences, allocs);
    report("same_offsets", same_offsets, detail);
    report("aligned_256", aligned);
    report("metered_total_is_real_off", total_equal);
    report("metering_pointer_non_null", nonnull);
    report("one_byte_less_is_exhausted", one_less_fails);
    report("exact_size_fits", exact_fits);

    // Arena::measure through the public helper gives the same number as a hand-driven metering arena
    {
        const std::vector<size_t> sizes = {3, 0, 70000, 256, 1};
        size_t want = 0;
        for (size_t b : sizes) want = ((want + 255) & ~size_t(255)) + b;
        report("measure", Arena::measure([&](Arena& a) { for (size_t b : sizes) (void)a.alloc(b); }) == want);
    }

    // carve(): the layout runs exactly twice, reserve exactly once with the metered size
    {
        Arena a;
        int runs = 0;
        char* last = nullptr;
        auto layout = [&](Arena& ar) { ++runs; (void)ar.alloc(1000); (void)ar.alloc(0); last = static_cast<char*>(ar.alloc(5000)); };
        bevgen::g_reserves = bevgen::g_mallocs = 0;
        a.carve(layout);
        const size_t need = 1024 + 5000;
        report("carve_runs_layout_twice_reserves_once",
               runs == 2 && bevgen::g_reserves == 1 && bevgen::g_last_reserve == need && a.off == need && a.cap == need && last == a.base + 1024 && !a.metering);
        // ... and does not reallocate when the capacity already suffices (a smaller layout, then the same one again)
        char* base = a.base;
        auto smaller = [&](Arena& ar) { (void)ar.alloc(10); };
        a.carve(smaller);
        a.carve(layout);
        report("carve_keeps_a_sufficient_slab", bevgen::g_mallocs == 1 && a.base == base && a.cap == need && bevgen::g_reserves == 3);
        // ... and grows when it does not
        auto larger = [&](Arena& ar) { (void)ar.alloc(need + 1); };
        a.carve(larger);
        report("carve_grows", bevgen::g_mallocs == 2 && a.cap == need + 1);
        a.release();
    }

    // carve()'s equality check fires for a layout that allocates differently on its second run
    for (int more = 0; more < 2; ++more) {
        Arena a;
        int runs = 0;
        bool fired = false;
        try {
            a.carve([&](Arena& ar) {
                ++runs;
                (void)ar.alloc(4096);
                if ((runs == 2) == (more == 1)) (void)ar.alloc(8);   // more = 1: the real run takes more (exhaustion); more = 0: it takes less (the equality check)
            });
        } catch (const bevgen::Error& e) {
            fired = more ? strstr(e.what(), "workspace arena exhausted") != nullptr : strstr(e.what(), "must allocate the same sequence on both runs") != nullptr;
        }
        report(more ? "carve_rejects_a_larger_second_run" : "carve_rejects_a_smaller_second_run", fired && runs == 2);
        a.release();
    }
    return g_failed;
}

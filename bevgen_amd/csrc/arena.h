// Workspace arena: a bump allocator over one device slab.  Host-only header (no HIP header): tests/host/arena_check.cpp exercises it on the CPU with a malloc-backed
// reserve / release; the library's are in context.cpp.
#pragma once
#include <cstddef>
#include <cstdint>

#include "error.h"

namespace bevgen {

// The workspace of a call is carved from the arena; nothing is allocated on the sampling path.
//
// THE WORKSPACE RULE.  A call describes its workspace once, as a layout function `void(Arena&)`, and hands it to carve().  carve() runs the layout TWICE: first on a
// metering arena (no memory, only offsets) to learn the size, then - after reserve(that size) and reset() - on the real one.  Running twice is safe because a layout
// function only takes from the arena it is given and stores the pointers in a plain struct: it issues no launch, no memset and no memcpy, touches no context state
// other than that struct, and never branches on a pointer it got from the arena (it branches on the condition that decided the allocation).  Compute code below a
// carve() receives the struct and asks the arena for nothing.
struct Arena {
    char* base = nullptr;
    size_t cap = 0, off = 0;
    bool metering = false;   // alloc() hands out fake addresses and never reports exhaustion: `off` ends at the bytes a real arena needs for the same sequence
    void reserve(size_t bytes);   // grows (free + allocate: the base moves) when bytes > cap
    void release();
    void reset() { off = 0; }
    void* alloc(size_t bytes) {
        const size_t a = (off + 255) & ~size_t(255);
        if (!metering && a + bytes > cap) fail(-4 /* BEVGEN_ERR_INTERNAL */, "workspace arena exhausted: need %zu more bytes (capacity %zu)", a + bytes - cap, cap);
        off = a + bytes;
        return base + a;
    }
    template <class T> T* get(size_t count) { return reinterpret_cast<T*>(alloc(count * sizeof(T))); }

    // bytes a real arena needs for `layout`
    template <class F> static size_t measure(F&& layout) {
        Arena m;
        m.metering = true;
        m.base = reinterpret_cast<char*>(uintptr_t(256));   // non-null and 256-aligned: a layout that stores or offsets a pointer behaves as on the real arena
        layout(m);
        return m.off;
    }
    template <class F> void carve(F&& layout) {
        const size_t need = measure(layout);
        reserve(need);
        reset();
        layout(*this);
        BG_REQUIRE(off == need, "workspace layout took %zu bytes after metering %zu: a layout function must allocate the same sequence on both runs", off, need);
    }
};

}  // namespace bevgen

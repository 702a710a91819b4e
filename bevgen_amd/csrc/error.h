// Error handling of libbevgen_hip: C++ exceptions inside, translated to int codes at the C-ABI.  Host-only: no HIP header.
#pragma once
#include <cstdarg>
#include <cstdio>
#include <stdexcept>
#include <string>

namespace bevgen {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

[[noreturn]] inline void fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    throw Error(code, buf);
}

#define BG_REQUIRE(cond, ...)                      \
    do {                                           \
        if (!(cond)) ::bevgen::fail(-1, __VA_ARGS__); \
    } while (0)

}  // namespace bevgen

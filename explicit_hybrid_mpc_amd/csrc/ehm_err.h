// The error channel of a translation unit: the message its ehm_*_last_error returns.  Every unit
// keeps a thread_local one of its own (include/ehmpc.h says which entry point reports where); the
// format attribute has the compiler check every refusal's arguments against its specifiers.  Plain
// C++ (tests/native/verdict_host_main.cpp drives it under the sanitizers).
#pragma once

#include <cstdarg>
#include <cstdio>
#include <string>

struct ehm_err_channel {
    std::string msg;

    // sets the message (cut at 511 characters) and returns `code`
    __attribute__((format(printf, 3, 4))) int fail(int code, const char* fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        vfail(code, fmt, ap);
        va_end(ap);
        return code;
    }
    // the same for a function that forwards its own variable arguments
    __attribute__((format(printf, 3, 0))) int vfail(int code, const char* fmt, va_list ap) {
        char buf[512];
        vsnprintf(buf, sizeof buf, fmt, ap);
        msg = buf;
        return code;
    }
    const char* c_str() const { return msg.c_str(); }
};

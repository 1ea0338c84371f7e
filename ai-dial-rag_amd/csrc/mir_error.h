// set_error's declaration and MIR_REQUIRE, nothing of HIP: vec_scoped_layout.h builds with any C++ compiler.  common.h includes it.
#pragma once
#include <stdint.h>

#include "../../include/miretr.h"

namespace mir {

// thread-local error text behind mir_last_error()
void set_error(const char *fmt, ...) __attribute__((format(printf, 1, 2)));

#define MIR_REQUIRE(cond, ...)                                                                     \
    do {                                                                                           \
        if (!(cond)) {                                                                             \
            ::mir::set_error(__VA_ARGS__);                                                         \
            return MIR_ERR_INVALID;                                                                \
        }                                                                                          \
    } while (0)

}  // namespace mir

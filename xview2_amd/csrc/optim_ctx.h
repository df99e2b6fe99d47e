// The gradient guard of the calling host thread (include/xv2.h "gradient guard", xv2_optim_guard_ctx): the device record the NEXT
// optimizer entry point reads its clip coefficient and its skip flag from.  Plain C++ (no HIP types).
#pragma once

namespace xv2 {

// byte layout of the record (include/xv2.h): the kernels index it as 32-bit words
constexpr int GUARD_NORM = 0;          // float
constexpr int GUARD_COEF = 1;          // float
constexpr int GUARD_SKIP = 2;          // int32
constexpr int GUARD_SKIPPED_ROW = 3;   // int32
constexpr int GUARD_STEPS64 = 2;       // int64 index: steps, clipped, skipped at 2, 3, 4
constexpr int GUARD_NORM_MAX = 10;     // float

const float*& optim_guard_ctx();       // thread-local (errors.cpp)

// every optimizer entry point holds one: the guard named by xv2_optim_guard_ctx() serves exactly ONE call and is cleared when
// that call returns, whatever it returns - a guard can never leak into a later step (AmaxGuard's lifetime, amax_ctx.h)
struct OptimGuardScope {
    const float* guard;
    OptimGuardScope() : guard(optim_guard_ctx()) {}
    ~OptimGuardScope() { optim_guard_ctx() = nullptr; }
    OptimGuardScope(const OptimGuardScope&) = delete;
    OptimGuardScope& operator=(const OptimGuardScope&) = delete;
};

}  // namespace xv2

// cnf_api.h — what the files that define C-ABI entry points (include/cnf.h) share: the error text behind
// cnf_last_error, the HIP error check and the exception-to-code wrapper. Internal; no GPU code here.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <stdexcept>
#include <string>

#include "../../include/cnf.h"

namespace cnf {

// keeps msg as the calling thread's cnf_last_error text and returns code (the string itself: cnf_runtime.cpp)
int set_error(int code, const char* msg);
inline int fail(int code, const std::string& msg) { return set_error(code, msg.c_str()); }

struct HipError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

inline void hip_check(hipError_t e, const char* what) {
    if (e != hipSuccess) throw HipError(std::string(what) + ": " + hipGetErrorString(e));
}
inline void check_launch() { hip_check(hipGetLastError(), "kernel launch"); }

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// the code and the error text of the exception in flight
inline int caught() {
    try {
        throw;
    } catch (const std::invalid_argument& e) {
        return fail(CNF_E_INVALID, e.what());
    } catch (const HipError& e) {
        return fail(CNF_E_HIP, e.what());
    } catch (const std::exception& e) {
        return fail(CNF_E_STATE, e.what());
    } catch (...) {
        return fail(CNF_E_STATE, "unknown error");
    }
}

}  // namespace cnf

// the body of an entry point that returns a status code: what it throws becomes the code and the error text
#define CNF_TRY try {
#define CNF_CATCH \
    }             \
    catch (...) { return ::cnf::caught(); }

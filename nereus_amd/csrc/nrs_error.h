// nrs_error.h — the error plumbing of the library without a HIP include: the NRS_* codes, the thread's last error text, fail() and
// NRSCHK.  nrs_ctx_base.h adds HIPCHK on top; the host components (nrs_host_bodies.h, nrs_host_settings.h, nrs_host_slab.h,
// nrs_host_state.h, nrs_host_plan.h, nrs_host_solver.h) need only this, so a plain host compiler builds them.
#pragma once
#include <string>

#include "../../include/nereus_hip.h"

namespace nrs {

extern thread_local std::string g_err; // defined in nrs_abi.hip
static inline int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}
#define NRSCHK(expr)              \
    do {                          \
        int r_ = (expr);          \
        if (r_ != NRS_OK) return r_; \
    } while (0)

} // namespace nrs

// nrs_host_bodies.h — the pose table of the kinematic boundary bodies (DESIGN.md "Kinematic boundary bodies"): host state in double,
// no HIP.  Body 0 is the static world; n = 0: no assignment.  The table is "moving" while a body has a velocity or a pose was set
// since the last rebuild of the boundary tables (dirty).  The context (nrs_ctx_impl.h) rounds the poses to SReal and launches.
#pragma once
#include <cmath>
#include <cstdint>

#include "nrs_error.h"

namespace nrs {

struct BodyPoses {
    struct Body { double c[3], x[3], q[4], v[3], w[3]; }; // rest centroid, position, orientation (w, x, y, z), velocity, angular velocity
    uint32_t n = 0;
    Body b[NRS_MAX_BODIES];
    bool dirty = false;

    static bool has_velocity(const Body &o) { return o.v[0] != 0.0 || o.v[1] != 0.0 || o.v[2] != 0.0 || o.w[0] != 0.0 || o.w[1] != 0.0 || o.w[2] != 0.0; }
    bool displaced() const
    {
        for (uint32_t k = 1; k < n; ++k) {
            const Body &o = b[k];
            if (o.x[0] != o.c[0] || o.x[1] != o.c[1] || o.x[2] != o.c[2] || o.q[0] != 1.0 || o.q[1] != 0.0 || o.q[2] != 0.0 || o.q[3] != 0.0) return true;
        }
        return false;
    }
    bool moving() const
    {
        if (!n) return false;
        if (dirty) return true;
        for (uint32_t k = 1; k < n; ++k) if (has_velocity(b[k])) return true;
        return false;
    }
    void clear() { n = 0; dirty = false; }
    // a new assignment: every body at rest at the centroid of its particles (sum[k] over cnt[k] of them), identity orientation
    void init(uint32_t nbodies, const double (*sum)[3], const uint64_t *cnt)
    {
        for (uint32_t k = 0; k < nbodies; ++k) {
            Body &o = b[k];
            for (int a = 0; a < 3; ++a) {
                o.c[a] = cnt[k] ? sum[k][a] / (double)cnt[k] : 0.0;
                o.x[a] = o.c[a]; o.v[a] = 0.0; o.w[a] = 0.0;
            }
            o.q[0] = 1.0; o.q[1] = o.q[2] = o.q[3] = 0.0;
        }
        n = nbodies;
    }
    int check(uint32_t body) const
    {
        if (!n) return fail(NRS_E_INVALID, "the context has no boundary bodies (nrs_set_boundary_bodies first)");
        if (body == 0) return fail(NRS_E_INVALID, "body 0 is the static world");
        if (body >= n) return fail(NRS_E_INVALID, "unknown body");
        return NRS_OK;
    }
    int set_velocity(uint32_t body, const double *v, const double *omega)
    {
        NRSCHK(check(body));
        for (int a = 0; a < 3; ++a)
            if (!std::isfinite(v[a]) || !std::isfinite(omega[a])) return fail(NRS_E_INVALID, "body velocity must be finite");
        for (int a = 0; a < 3; ++a) { b[body].v[a] = v[a]; b[body].w[a] = omega[a]; }
        return NRS_OK;
    }
    int set_pose(uint32_t body, const double *x, const double *q)
    {
        NRSCHK(check(body));
        const double nq = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        if (!std::isfinite(x[0]) || !std::isfinite(x[1]) || !std::isfinite(x[2]) || !std::isfinite(nq)) return fail(NRS_E_INVALID, "body pose must be finite");
        if (!(nq > 0.0)) return fail(NRS_E_INVALID, "zero quaternion");
        for (int a = 0; a < 3; ++a) b[body].x[a] = x[a];
        for (int a = 0; a < 4; ++a) b[body].q[a] = q[a] / nq;
        dirty = true;
        return NRS_OK;
    }
    int get_pose(uint32_t body, double *x, double *q) const
    {
        NRSCHK(check(body));
        for (int a = 0; a < 3; ++a) x[a] = b[body].x[a];
        for (int a = 0; a < 4; ++a) q[a] = b[body].q[a];
        return NRS_OK;
    }
    // x += dt v; q = exp(dt omega / 2) q (the exact exponential map, identity when |omega| = 0), renormalised
    static void advance_body(Body &o, double dt)
    {
        for (int a = 0; a < 3; ++a) o.x[a] += dt * o.v[a];
        const double wn = std::sqrt(o.w[0] * o.w[0] + o.w[1] * o.w[1] + o.w[2] * o.w[2]);
        if (wn == 0.0) return;
        const double half = 0.5 * dt * wn, s = std::sin(half) / wn;
        const double e[4] = {std::cos(half), s * o.w[0], s * o.w[1], s * o.w[2]};
        const double *q = o.q;
        double r[4] = {e[0] * q[0] - e[1] * q[1] - e[2] * q[2] - e[3] * q[3], e[0] * q[1] + e[1] * q[0] + e[2] * q[3] - e[3] * q[2],
                       e[0] * q[2] - e[1] * q[3] + e[2] * q[0] + e[3] * q[1], e[0] * q[3] + e[1] * q[2] - e[2] * q[1] + e[3] * q[0]};
        const double nr = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3]);
        for (int a = 0; a < 4; ++a) o.q[a] = r[a] / nr;
    }
    // one step of every body that has a velocity
    void advance(double dt)
    {
        for (uint32_t k = 1; k < n; ++k)
            if (has_velocity(b[k])) advance_body(b[k], dt);
    }
    // the rotation matrix of body k's orientation, row-major
    void rotation(uint32_t k, double *rot) const
    {
        const double w = b[k].q[0], x = b[k].q[1], y = b[k].q[2], z = b[k].q[3];
        rot[0] = 1.0 - 2.0 * (y * y + z * z); rot[1] = 2.0 * (x * y - w * z); rot[2] = 2.0 * (x * z + w * y);
        rot[3] = 2.0 * (x * y + w * z); rot[4] = 1.0 - 2.0 * (x * x + z * z); rot[5] = 2.0 * (y * z - w * x);
        rot[6] = 2.0 * (x * z - w * y); rot[7] = 2.0 * (y * z + w * x); rot[8] = 1.0 - 2.0 * (x * x + y * y);
    }
};

} // namespace nrs

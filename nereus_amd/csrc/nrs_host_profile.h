// nrs_host_profile.h — the stage timer behind nrs_set_profiling / nrs_stage_ms: a pool of event pairs recorded around the launches of
// a stage, resolved into per-stage times and launch counts when somebody asks (collect synchronises the stream).
#pragma once
#include "nrs_ctx_base.h"

namespace nrs {

struct StageTimer {
    struct Ev { int stage; Event a, b; bool cont; };
    std::vector<Ev> pool;
    size_t used = 0; // pairs recorded since the last collect
    float stageMs[NRS_STAGE_COUNT] = {0};
    uint32_t stageLaunches[NRS_STAGE_COUNT] = {0};
    bool open = false;

    // cont: second part of a stage whose first part ran earlier (time is added, the launch count is not)
    int begin(int stage, bool cont, uint32_t mask, hipStream_t stream)
    {
        open = (mask >> stage) & 1u;
        if (!open) return NRS_OK;
        if (used == pool.size()) {
            Ev e; e.stage = stage;
            HIPCHK(hipEventCreate(&e.a.e));
            HIPCHK(hipEventCreate(&e.b.e));
            pool.push_back(std::move(e));
        }
        pool[used].stage = stage;
        pool[used].cont = cont;
        HIPCHK(hipEventRecord(pool[used].a, stream));
        return NRS_OK;
    }
    int end(hipStream_t stream)
    {
        if (!open) return NRS_OK;
        open = false;
        HIPCHK(hipEventRecord(pool[used].b, stream));
        ++used;
        return NRS_OK;
    }
    int collect(hipStream_t stream)
    {
        if (!used) return NRS_OK;
        HIPCHK(hipStreamSynchronize(stream));
        for (size_t i = 0; i < used; ++i) {
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, pool[i].a, pool[i].b));
            stageMs[pool[i].stage] += ms;
            stageLaunches[pool[i].stage] += pool[i].cont ? 0 : 1;
        }
        used = 0;
        return NRS_OK;
    }
    int reset(hipStream_t stream) // a new mask starts from zero
    {
        NRSCHK(collect(stream));
        std::memset(stageMs, 0, sizeof(stageMs));
        std::memset(stageLaunches, 0, sizeof(stageLaunches));
        return NRS_OK;
    }
    int read(int stage, float *ms, uint32_t *launches, hipStream_t stream)
    {
        if (stage < 0 || stage >= NRS_STAGE_COUNT) return fail(NRS_E_INVALID, "bad stage");
        NRSCHK(collect(stream)); // resolves the pending event pairs (synchronizes the stream)
        *ms = stageMs[stage];
        if (launches) *launches = stageLaunches[stage];
        return NRS_OK;
    }
};

} // namespace nrs

// headless.cpp — drives Nereus::SPH / Nereus::IISPH through the class API only (what main.cpp does, minus
// the viewer) and dumps the state for the parity tests.
//
//   headless params  <sesph|iisph> <out.bin>                    constructor-default SphSimParams bytes
//   headless run     <sesph|iisph> <in.bin> <steps> <out.bin>   particles/boundaries from a file (also pcisph: the reference's
//                                                               stub, pcisph-solve: PCISPH::setPressureSolve(true), pbf:
//                                                               Nereus::PBF with its default settings, and pbf-full: PBF with
//                                                               XSPH 0.01, the tensile correction k = 1e-4, dq = 0.2 and
//                                                               vorticity confinement eps_v = 0.01; dfsph: Nereus::DFSPH with
//                                                               its default settings, and dfsph-akinci: DFSPH with
//                                                               setAkinciSurface(1, 1))
//   headless resume  <sesph|iisph> <in.bin> <steps_a> <steps_b> <ckpt> <out.bin>   run steps_a, saveState, then a NEW
//                                                               solver loadState()s and runs steps_b (boundaries re-set)
//   headless cfl     sesph <in.bin> <steps> <out.bin>           run with setAdaptiveTimestep(true)
//   headless mainscene <sesph|iisph> <steps> <out.bin>          main.cpp:533-553: generateParticleCube + sampleBox +
//                                                               getVbi + updateGpuBoundaries, gravity as given
//   headless piston  <solver> <steps> <out.bin>                 a box of fluid (generateParticleCube) in the sampled box, and one
//                                                               wall, a plate of boundary particles behind the fluid that is body 1
//                                                               and moves at 1 m/s along +x (setBoundaryBodies / setBodyVelocity);
//                                                               the dumped bi are the rest positions, the plate last
//   headless lattice <solver> <in.bin> <steps> <ox> <oy> <oz> <spacing> <dx> <dy> <dz> <out.lat>
//                                                               as run, then the density (fluid only) on the dx x dy x dz nodes
//                                                               origin + idx * spacing (SPH::sampleLattice / getSampledDensity)
//                                                               out.lat: u32 dx, dy, dz, u32 precision (32 | 64), SReal[dx * dy * dz]
//   headless surface <solver> <in.bin> <steps> <ox> <oy> <oz> <spacing> <dx> <dy> <dz> <iso> <out.obj>
//                                                               as run, then the surface density = iso on that lattice
//                                                               (SPH::extractSurface) as a Wavefront OBJ: "v x y z" lines, then
//                                                               "f a b c" lines with 1-based vertex numbers, wound outwards
//   headless surface ... <iso> <out.obj> --aniso [support]      the same with the anisotropic kernels (SPH::extractSurfaceAniso): <iso> is a
//                                                               value of the colour field (0.5); support: a length, default (and 0) h
//   headless diffuse <solver> <in.bin> <steps> <out.dif>        as run with SPH::stepDiffuse after every update (capacity 2^20, seed 0,
//                                                               the ranges below), then the living diffuse set (SPH::getDiffuse)
//                                                               out.dif: u32 count, u32 precision (32 | 64), pos4[count] (w = lifetime),
//                                                               vel4[count], u32 kind[count] (0 spray, 1 foam, 2 bubble)
//   headless faucet <solver> <steps> <out.bin>                  no input: an empty solver with the constructor's parameters and no walls, a disc
//                                                               emitter (SPH::setEmitter: centre (0, -0.9, 0), pointing down, radius 2.5
//                                                               rest spacings, 4 m/s) and a domain sink (SPH::setSinks); <steps> updates,
//                                                               then out.bin: u32 n, u32 precision (32 | 64), u64 emitted, u64 dropped,
//                                                               u64 removed, u64 culls, pos4[n], vel4[n]
//   headless track <solver> <steps> <out.txt> [kappa]           the faucet scene with SPH::setParticleTracking(true) and two touching disc
//                                                               emitters, red (slot 0, left) and blue (slot 1, right); SPH::diffuseColors
//                                                               with kappa (default 0.05; 0: never) on r, g, b after every update;
//                                                               out.txt: "id birth x y z r g b a" per living particle
//   headless colours <solver> <steps> <track 0|1> <out.txt>     the shipped cube with colour.r = the particle's number, <steps> updates (tracking:
//                                                               then a context rebuilt to grow and one more); out.txt per number k:
//                                                               "k slot id r", slot from SPH::locateParticles (k without tracking), r =
//                                                               getHostCol()[4 * slot]
//   headless mesh <in.obj> <spacing> <fill|shell> <out.bin>     no solver kind: the "v" and "f" lines of a Wavefront OBJ (polygons fanned from their
//                                                               first corner, "a/b/c" corners by their first number, negative numbers
//                                                               from the end; wound outwards) sampled on ss::meshLattice(vertices, spacing);
//                                                               shell: ss::sampleMesh (one layer on the surface); fill: SPH::emitMesh with
//                                                               clearance spacing / 2 and no velocity into an empty solver.
//                                                               out.bin: u32 n, u32 precision (32 | 64), pos4[n]
//   headless viscous <nu> <nu_b> <steps> <out.bin>              no solver kind: Nereus::DFSPH with setImplicitViscosity(nu, nu_b, 1e-3, 1, 0) on the
//                                                               mainscene dam break (the cube in the sampled box); out.bin as run's, iters =
//                                                               the density solve's
// in.bin : u32 n, u32 nb, then pos4[n], vel4[n], bi4[nb], vbi[nb] (SReal)
// out.bin: u32 n, u32 nb, u32 iters, u32 sizeof(params), params, pos4[n], vel4[n], pressure[n], bi4[nb], vbi[nb]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "common.h"
#include "nereus_hip.h"
#include "iisph/iisph.h"
#include "dfsph/dfsph.h"
#include "pbf/pbf.h"
#include "pcisph/pcisph.h"
#include "sph.h"
#include <sph_boundary_particles/boundary_forces.h>
#include <sph_boundary_particles/ss.h>

static void die(const char *m) { std::fprintf(stderr, "headless: %s\n", m); std::exit(2); }

static void dump(const char *path, Nereus::SPH *s, unsigned iters, const std::vector<SVec4> &bi, const std::vector<SReal> &vbi)
{
    FILE *f = std::fopen(path, "wb");
    if (!f) die("cannot open output");
    const unsigned n = s->getNumParticles(), nb = (unsigned)bi.size(), ps = sizeof(SphSimParams);
    const SphSimParams P = s->getParams();
    std::fwrite(&n, 4, 1, f); std::fwrite(&nb, 4, 1, f); std::fwrite(&iters, 4, 1, f); std::fwrite(&ps, 4, 1, f);
    std::fwrite(&P, ps, 1, f);
    std::fwrite(s->getHostPos(), sizeof(SReal) * 4, n, f);
    std::fwrite(s->getHostVel(), sizeof(SReal) * 4, n, f);
    std::fwrite(s->getHostPressure(), sizeof(SReal), n, f);
    if (nb) { std::fwrite(bi.data(), sizeof(SVec4), nb, f); std::fwrite(vbi.data(), sizeof(SReal), nb, f); }
    std::fclose(f);
}

// the triangle mesh of a Wavefront OBJ: every "v x y z" line a vertex, every "f ..." line a polygon, fanned
static void read_obj(const char *path, std::vector<double> &vertices, std::vector<uint32_t> &triangles)
{
    FILE *f = std::fopen(path, "r");
    if (!f) die("cannot open input");
    std::vector<char> line(1 << 16);
    while (std::fgets(line.data(), (int)line.size(), f)) {
        char *p = line.data();
        while (*p == ' ' || *p == '\t') ++p;
        if (p[0] == 'v' && (p[1] == ' ' || p[1] == '\t')) {
            ++p;
            for (int a = 0; a < 3; ++a) {
                char *end = nullptr;
                vertices.push_back(std::strtod(p, &end));
                if (end == p) die("obj: a vertex line with fewer than three numbers");
                p = end;
            }
        } else if (p[0] == 'f' && (p[1] == ' ' || p[1] == '\t')) {
            ++p;
            std::vector<uint32_t> corner;
            for (;;) {
                char *end = nullptr;
                const long long k = std::strtoll(p, &end, 10);
                if (end == p) break;
                const long long nv = (long long)(vertices.size() / 3), idx = k > 0 ? k - 1 : nv + k;
                if (k == 0 || idx < 0 || idx >= nv) die("obj: a face names a vertex that is not there (yet)");
                corner.push_back((uint32_t)idx);
                p = end;
                while (*p && *p != ' ' && *p != '\t' && *p != '\n' && *p != '\r') ++p; // (the /vt/vn part)
            }
            if (corner.size() < 3) die("obj: a face with fewer than three corners");
            for (size_t c = 1; c + 1 < corner.size(); ++c) {
                triangles.push_back(corner[0]); triangles.push_back(corner[c]); triangles.push_back(corner[c + 1]);
            }
        }
    }
    std::fclose(f);
}

int main(int argc, char **argv)
{
    if (argc < 4) die("usage: see source header");
    const std::string mode = argv[1], kind = argv[2];
    if (mode == "vbi") { // headless vbi <bi.f32 (xyzw)> <h> <out.f32>: getVbi (device) then getVbiHost (host cross-check)
        if (argc < 5) die("vbi needs <bi.f32> <h> <out.f32>");
        FILE *f = std::fopen(argv[2], "rb");
        if (!f) die("cannot open input");
        std::fseek(f, 0, SEEK_END);
        const size_t nb = (size_t)std::ftell(f) / sizeof(SVec4);
        std::fseek(f, 0, SEEK_SET);
        std::vector<SVec4> b(nb);
        if (nb && std::fread(b.data(), sizeof(SVec4), nb, f) != nb) die("short input");
        std::fclose(f);
        std::vector<SReal> dev, host;
        const SReal h = (SReal)std::atof(argv[3]);
        sample_spheres::boundary_forces::getVbi(dev, b, h);
        sample_spheres::boundary_forces::getVbiHost(host, b, h);
        FILE *o = std::fopen(argv[4], "wb");
        if (!o) die("cannot open output");
        std::fwrite(dev.data(), sizeof(SReal), nb, o);
        std::fwrite(host.data(), sizeof(SReal), nb, o);
        std::fclose(o);
        return 0;
    }
    if (mode == "mesh") {
        if (argc < 6) die("mesh needs <in.obj> <spacing> <fill|shell> <out.bin>");
        std::vector<double> vertices;
        std::vector<uint32_t> triangles;
        read_obj(argv[2], vertices, triangles);
        const double spacing = std::strtod(argv[3], nullptr);
        const std::string what = argv[4];
        std::vector<SVec4> out;
        if (what == "shell") {
            sample_spheres::ss::sampleMesh(out, vertices, triangles, spacing);
        } else if (what == "fill") {
            const nrs_lattice L = sample_spheres::ss::meshLattice(vertices, spacing);
            const nrs_mesh mesh = {vertices.data(), (uint64_t)(vertices.size() / 3), triangles.data(), (uint64_t)(triangles.size() / 3)};
            const nrs_mesh_rule rule = {NRS_MESH_INSIDE, 0u, spacing / 2, INFINITY};
            uint64_t count = 0; // (how much room the solver needs)
            if (nrs_mesh_particles(-1, (int)(8 * sizeof(SReal)), &mesh, &L, &rule, nullptr, 0, &count) != 0) die(nrs_last_error());
            Nereus::SPH fluid;
            fluid._initialize();
            if (count) fluid.reserveParticles((SUint)count);
            const double vel[3] = {0.0, 0.0, 0.0};
            const SUint dims[3] = {L.dims[0], L.dims[1], L.dims[2]};
            const SUint added = fluid.emitMesh(vertices, triangles, L.origin, L.spacing, dims, spacing / 2, vel);
            if (added != count || fluid.getNumParticles() != added) die("emitMesh: not the count nrs_mesh_particles gives");
            const SVec4 *hp = (const SVec4 *)fluid.getHostPos();
            out.assign(hp, hp + added);
        } else {
            die("mesh: fill or shell");
        }
        FILE *o = std::fopen(argv[5], "wb");
        if (!o) die("cannot open output");
        const unsigned head[2] = {(unsigned)out.size(), (unsigned)(8 * sizeof(SReal))};
        std::fwrite(head, sizeof(unsigned), 2, o);
        if (!out.empty()) std::fwrite(out.data(), sizeof(SVec4), out.size(), o);
        std::fclose(o);
        std::printf("mesh: %zu vertices, %zu triangles, %zu particles (%s)\n", vertices.size() / 3, triangles.size() / 3, out.size(), what.c_str());
        return 0;
    }
    if (mode == "viscous") {
        if (argc < 6) die("viscous needs <nu> <nu_b> <steps> <out.bin>");
        Nereus::DFSPH fluid;
        fluid.setImplicitViscosity(std::atof(argv[2]), std::atof(argv[3]), 1e-3, 1, 0);
        fluid._initialize();
        fluid.generateParticleCube(make_SVec4(-0.4f, 0.04f, 0.5f, 1.f), make_SVec4(0.5f, 0.5f, 0.5f, 1.f), make_SVec4(0, 0, 0, 0));
        std::vector<SVec4> walls;
        std::vector<SReal> volumes;
        sample_spheres::ss::sampleBox(walls, make_SVec3(-1, -1, -1), make_SVec3(3.f, 3.f, 3.f), 0.02);
        sample_spheres::boundary_forces::getVbi(volumes, walls, fluid.getInteractionRadius());
        fluid.setNumBoundaries(walls.size());
        fluid.setBi((SReal *)walls.data());
        fluid.setVbi(volumes.data());
        fluid.updateGpuBoundaries(walls.size());
        const int steps = std::atoi(argv[4]);
        for (int s = 0; s < steps; ++s) fluid.update();
        SUint cg = 0;
        double residual = 0.0, rhs = 0.0;
        const bool on = fluid.implicitViscosityInfo(&cg, &residual, &rhs);
        std::printf("viscous: %s, %u CG iterations in the last step, |r| / |b| = %.3g\n", on ? "on" : "off", cg, rhs > 0.0 ? residual / rhs : 0.0);
        dump(argv[5], &fluid, fluid.getLastIterations(), walls, volumes);
        fluid._finalize();
        return 0;
    }
    const bool iisph = kind == "iisph", pcisphSolve = kind == "pcisph-solve", pcisph = kind == "pcisph" || pcisphSolve;
    const bool pbfFull = kind == "pbf-full", pbf = kind == "pbf" || pbfFull;
    const bool dfsphAkinci = kind == "dfsph-akinci", dfsph = kind == "dfsph" || dfsphAkinci;
    Nereus::SPH *sim = iisph ? (Nereus::SPH *)new Nereus::IISPH()
                             : (pcisph ? (Nereus::SPH *)new Nereus::PCISPH()
                                       : (pbf ? (Nereus::SPH *)new Nereus::PBF() : (dfsph ? (Nereus::SPH *)new Nereus::DFSPH() : new Nereus::SPH())));
    if (pcisphSolve) static_cast<Nereus::PCISPH *>(sim)->setPressureSolve(true);
    if (pbfFull) {
        Nereus::PBF *p = static_cast<Nereus::PBF *>(sim);
        p->setSolverSettings((SReal)0.01, 2, (SReal)0.01, (SReal)0.01);
        p->setTensileCorrection((SReal)1e-4, (SReal)0.2);
        p->setVorticityConfinement((SReal)0.01);
    }
    if (dfsphAkinci) static_cast<Nereus::DFSPH *>(sim)->setAkinciSurface((SReal)1.0, (SReal)1.0);
    sim->_initialize();
    std::vector<SVec4> bi;
    std::vector<SReal> vbi;
    unsigned iters = 0;
    if (mode == "params") {
        dump(argv[3], sim, 0, bi, vbi);
    } else if (mode == "faucet") {
        if (argc < 5) die("faucet needs <steps> <out.bin>");
        const int steps = std::atoi(argv[3]);
        const SphSimParams &P = sim->getParams();
        nrs_emitter em;
        std::memset(&em, 0, sizeof(em));
        em.shape = NRS_EMITTER_DISC; em.enabled = 1;
        em.center[1] = -0.9; em.direction[1] = -1.0;
        em.half_extent[0] = 2.5 * std::cbrt((double)P.particleMass / (double)P.restDensity);
        em.speed = 4.0;
        nrs_sink_config sk;
        std::memset(&sk, 0, sizeof(sk));
        sk.flags = NRS_SINK_DOMAIN;
        sim->setEmitter(0, &em);
        sim->setSinks(&sk);
        for (int s = 0; s < steps; ++s) sim->update();
        unsigned long long emitted = 0, dropped = 0, removed = 0, culls = 0;
        sim->getEmitter(0, nullptr, &emitted, &dropped);
        sim->sinkCounts(&removed, &culls);
        const unsigned n = sim->getNumParticles();
        FILE *o = std::fopen(argv[4], "wb");
        if (!o) die("cannot open output");
        const unsigned head[2] = {n, (unsigned)(8 * sizeof(SReal))};
        const unsigned long long counts[4] = {emitted, dropped, removed, culls};
        std::fwrite(head, sizeof(unsigned), 2, o);
        std::fwrite(counts, sizeof(unsigned long long), 4, o);
        std::fwrite(sim->getHostPos(), sizeof(SReal) * 4, n, o);
        std::fwrite(sim->getHostVel(), sizeof(SReal) * 4, n, o);
        std::fclose(o);
        std::printf("faucet: %u particles after %d steps (%llu emitted, %llu removed)\n", n, steps, emitted, removed);
    } else if (mode == "track") {
        if (argc < 5) die("track needs <steps> <out.txt> [kappa]");
        const int steps = std::atoi(argv[3]);
        const double k = argc > 5 ? std::atof(argv[5]) : 0.05;
        const SphSimParams &P = sim->getParams();
        const double s0 = std::cbrt((double)P.particleMass / (double)P.restDensity);
        sim->setParticleTracking(true);
        nrs_sink_config sk;
        std::memset(&sk, 0, sizeof(sk));
        sk.flags = NRS_SINK_DOMAIN;
        sim->setSinks(&sk);
        for (int e = 0; e < 2; ++e) { // two touching jets: red on the left, blue on the right
            nrs_emitter em;
            std::memset(&em, 0, sizeof(em));
            em.shape = NRS_EMITTER_DISC; em.enabled = 1;
            em.center[0] = (e ? 2.5 : -2.5) * s0; em.center[1] = -0.9; em.direction[1] = -1.0;
            em.half_extent[0] = 2.5 * s0;
            em.speed = 4.0;
            sim->setEmitter((SUint)e, &em);
            sim->setEmitterColor(e, e ? make_SVec4(0, 0, 1, 1) : make_SVec4(1, 0, 0, 1));
        }
        const double kappa[4] = {k, k, k, 0.0};
        for (int s = 0; s < steps; ++s) {
            sim->update();
            if (k > 0.0) sim->diffuseColors(kappa);
        }
        const unsigned n = sim->getNumParticles();
        const SUint *ids = sim->getHostIds(), *birth = sim->getHostBirth();
        const SReal *x = sim->getHostPos(), *c = sim->getHostCol();
        FILE *o = std::fopen(argv[4], "w");
        if (!o) die("cannot open output");
        for (unsigned i = 0; i < n; ++i)
            std::fprintf(o, "%u %u %.9g %.9g %.9g %.9g %.9g %.9g %.9g\n", ids[i], birth[i], (double)x[4 * i], (double)x[4 * i + 1], (double)x[4 * i + 2],
                         (double)c[4 * i], (double)c[4 * i + 1], (double)c[4 * i + 2], (double)c[4 * i + 3]);
        std::fclose(o);
        std::printf("track: %u particles after %d steps\n", n, steps);
    } else if (mode == "colours") {
        if (argc < 6) die("colours needs <steps> <track 0|1> <out.txt>");
        const int steps = std::atoi(argv[3]);
        const bool track = std::atoi(argv[4]) != 0;
        sim->generateParticleCube(make_SVec4(-0.4, 0.04, 0.5, 1.0), make_SVec4(0.5, 0.5, 0.5, 1.0), make_SVec4(0, 0, 0, 0));
        const unsigned n = sim->getNumParticles();
        sim->setParticleTracking(track);
        SReal *col = sim->getCol();
        for (unsigned i = 0; i < n; ++i) { col[4 * i] = (SReal)i; col[4 * i + 1] = (SReal)0.5; col[4 * i + 2] = (SReal)0; col[4 * i + 3] = (SReal)1; }
        for (int s = 0; s < steps; ++s) sim->update();
        if (track) sim->reserveParticles(2 * MAX_PARTICLE_NUMBER); // a context rebuilt to grow keeps ids, births and colours
        if (track) sim->update();
        FILE *o = std::fopen(argv[5], "w");
        if (!o) die("cannot open output");
        const SReal *c = sim->getHostCol();
        std::vector<SUint> slotOf(n);
        for (unsigned k = 0; k < n; ++k) slotOf[k] = k;
        if (track) slotOf = sim->locateParticles(0, n);
        for (unsigned k = 0; k < n && k < 16 && track; ++k) slotOf[k] = sim->locateParticles(k, 1)[0]; // (one id at a time gives the same)
        const SUint *ids = track ? sim->getHostIds() : nullptr;
        for (unsigned k = 0; k < n; ++k) {
            const unsigned slot = slotOf[k];
            const unsigned id = track ? ids[slot] : k;
            std::fprintf(o, "%u %u %u %.9g\n", k, slot, id, (double)c[4 * slot]);
        }
        std::fclose(o);
    } else if (mode == "run" || mode == "frames" || mode == "lattice" || mode == "surface" || mode == "diffuse") {
        if (argc < 6) die("run needs <in.bin> <steps> <out.bin>");
        if (mode == "lattice" && argc < 13) die("lattice needs <in.bin> <steps> <ox> <oy> <oz> <spacing> <dx> <dy> <dz> <out.lat>");
        if (mode == "surface" && argc < 14) die("surface needs <in.bin> <steps> <ox> <oy> <oz> <spacing> <dx> <dy> <dz> <iso> <out.obj>");
        FILE *f = std::fopen(argv[3], "rb");
        if (!f) die("cannot open input");
        unsigned n = 0, nb = 0;
        if (std::fread(&n, 4, 1, f) != 1 || std::fread(&nb, 4, 1, f) != 1) die("short input");
        std::vector<SVec4> pos(n), vel(n);
        bi.resize(nb); vbi.resize(nb);
        if (n && (std::fread(pos.data(), sizeof(SVec4), n, f) != n || std::fread(vel.data(), sizeof(SVec4), n, f) != n)) die("short input");
        if (nb && (std::fread(bi.data(), sizeof(SVec4), nb, f) != nb || std::fread(vbi.data(), sizeof(SReal), nb, f) != nb)) die("short input");
        std::fclose(f);
        for (unsigned i = 0; i < n; ++i) sim->addNewParticle(pos[i], vel[i]);
        if (nb) {
            sim->setNumBoundaries(nb);
            sim->setBi((SReal *)bi.data());
            sim->setVbi(vbi.data());
            sim->updateGpuBoundaries(nb);
        }
        const int steps = std::atoi(argv[4]);
        if (mode == "frames") { // render-loop pattern: update(); draw(latestFrame()) — the frame may lag, never the solver
            sim->setAsyncReadback(true);
            unsigned long long last = 0;
            for (int s = 0; s < steps; ++s) {
                sim->update();
                SUint fn = 0;
                unsigned long long fstep = 0;
                const SReal *frame = sim->latestFrame(&fn, &fstep);
                if (!frame || fn != sim->getNumParticles()) die("latestFrame: no frame");
                if (fstep < last || fstep > (unsigned long long)(s + 1) || fstep + 2 < (unsigned long long)(s + 1)) die("latestFrame: stale or out of order");
                last = fstep;
            }
        } else if (mode == "diffuse") {
            nrs_diffuse_config dc;
            std::memset(&dc, 0, sizeof(dc));
            dc.capacity = 1u << 20;
            dc.tau_ta[0] = 0.1; dc.tau_ta[1] = 0.5;
            dc.tau_wc[0] = 0.1; dc.tau_wc[1] = 1.0;
            dc.tau_k[0] = 5e-4; dc.tau_k[1] = 4e-3;
            dc.k_ta = dc.k_wc = 3000.0;
            dc.lifetime[0] = 0.5; dc.lifetime[1] = 2.0;
            dc.k_buoyancy = 2.0; dc.k_drag = 0.8;
            dc.spray_below = 6; dc.bubble_above = 20;
            dc.max_per_particle = 3;
            sim->configureDiffuse(dc);
            for (int s = 0; s < steps; ++s) {
                sim->update();
                sim->stepDiffuse();
            }
        } else {
            for (int s = 0; s < steps; ++s) sim->update();
        }
        if (iisph) iters = static_cast<Nereus::IISPH *>(sim)->getLastIterations();
        if (pcisphSolve) iters = static_cast<Nereus::PCISPH *>(sim)->getLastIterations();
        if (pbf) iters = static_cast<Nereus::PBF *>(sim)->getLastIterations();
        if (dfsph) iters = static_cast<Nereus::DFSPH *>(sim)->getLastIterations();
        if (mode == "lattice") {
            const double h = std::strtod(argv[8], nullptr);
            const double origin[3] = {std::strtod(argv[5], nullptr), std::strtod(argv[6], nullptr), std::strtod(argv[7], nullptr)}, spacing[3] = {h, h, h};
            const SUint dims[3] = {(SUint)std::strtoul(argv[9], nullptr, 10), (SUint)std::strtoul(argv[10], nullptr, 10), (SUint)std::strtoul(argv[11], nullptr, 10)};
            sim->sampleLattice(origin, spacing, dims, NRS_FIELD_DENSITY);
            const std::vector<SReal> &rho = sim->getSampledDensity();
            if (rho.size() != (size_t)dims[0] * dims[1] * dims[2]) die("getSampledDensity: wrong size");
            FILE *o = std::fopen(argv[12], "wb");
            if (!o) die("cannot open output");
            const unsigned head[4] = {dims[0], dims[1], dims[2], (unsigned)(8 * sizeof(SReal))};
            std::fwrite(head, 4, 4, o);
            std::fwrite(rho.data(), sizeof(SReal), rho.size(), o);
            std::fclose(o);
        } else if (mode == "diffuse") {
            const SVec4 *dp = nullptr, *dv = nullptr;
            const SUint *dk = nullptr;
            const SUint count = sim->getDiffuse(&dp, &dv, &dk);
            FILE *o = std::fopen(argv[5], "wb");
            if (!o) die("cannot open output");
            const unsigned head[2] = {count, (unsigned)(8 * sizeof(SReal))};
            std::fwrite(head, sizeof(unsigned), 2, o);
            std::fwrite(dp, sizeof(SVec4), count, o);
            std::fwrite(dv, sizeof(SVec4), count, o);
            std::fwrite(dk, sizeof(SUint), count, o);
            std::fclose(o);
            std::printf("diffuse: %u particles after %d steps\n", count, steps);
        } else if (mode == "surface") {
            const double h = std::strtod(argv[8], nullptr);
            const double origin[3] = {std::strtod(argv[5], nullptr), std::strtod(argv[6], nullptr), std::strtod(argv[7], nullptr)}, spacing[3] = {h, h, h};
            const SUint dims[3] = {(SUint)std::strtoul(argv[9], nullptr, 10), (SUint)std::strtoul(argv[10], nullptr, 10), (SUint)std::strtoul(argv[11], nullptr, 10)};
            const bool aniso = argc > 14 && std::string(argv[14]) == "--aniso";
            if (argc > 14 && !aniso) die("surface: unknown option (--aniso [support])");
            if (aniso) {
                nrs_aniso_config ac;
                std::memset(&ac, 0, sizeof(ac));
                ac.support = argc > 15 ? std::strtod(argv[15], nullptr) : 0.0;
                ac.lambda = 0.9; ac.k_r = 4.0; ac.k_n = 0.5; ac.n_eps = 25;
                sim->extractSurfaceAniso(origin, spacing, dims, std::strtod(argv[12], nullptr), 0, &ac);
            } else {
                sim->extractSurface(origin, spacing, dims, std::strtod(argv[12], nullptr), 0);
            }
            const std::vector<SVec4> &v = sim->getSurfaceVertices();
            const std::vector<SUint> &t = sim->getSurfaceTriangles();
            if (v.size() != sim->getSurfaceNumVertices() || t.size() != 3 * (size_t)sim->getSurfaceNumTriangles()) die("extractSurface: wrong sizes");
            FILE *o = std::fopen(argv[13], "w");
            if (!o) die("cannot open output");
            std::fprintf(o, "# %s = %s, %zu vertices, %zu triangles\n", aniso ? "anisotropic colour field" : "density", argv[12], v.size(), t.size() / 3);
            const int digits = sizeof(SReal) == 8 ? 17 : 9; // enough to read every coordinate back bit for bit
            for (size_t i = 0; i < v.size(); ++i) std::fprintf(o, "v %.*g %.*g %.*g\n", digits, (double)v[i].x, digits, (double)v[i].y, digits, (double)v[i].z);
            for (size_t i = 0; i + 2 < t.size(); i += 3) std::fprintf(o, "f %u %u %u\n", t[i] + 1, t[i + 1] + 1, t[i + 2] + 1);
            std::fclose(o);
        } else {
            dump(argv[5], sim, iters, bi, vbi);
        }
    } else if (mode == "resume" || mode == "cfl") {
        FILE *f = std::fopen(argv[3], "rb");
        if (!f) die("cannot open input");
        unsigned n = 0, nb = 0;
        if (std::fread(&n, 4, 1, f) != 1 || std::fread(&nb, 4, 1, f) != 1) die("short input");
        std::vector<SVec4> pos(n), vel(n);
        bi.resize(nb); vbi.resize(nb);
        if (n && (std::fread(pos.data(), sizeof(SVec4), n, f) != n || std::fread(vel.data(), sizeof(SVec4), n, f) != n)) die("short input");
        if (nb && (std::fread(bi.data(), sizeof(SVec4), nb, f) != nb || std::fread(vbi.data(), sizeof(SReal), nb, f) != nb)) die("short input");
        std::fclose(f);
        auto setup = [&](Nereus::SPH *s, bool particles) {
            if (particles) for (unsigned i = 0; i < n; ++i) s->addNewParticle(pos[i], vel[i]);
            if (nb) { s->setNumBoundaries(nb); s->setBi((SReal *)bi.data()); s->setVbi(vbi.data()); s->updateGpuBoundaries(nb); }
        };
        if (mode == "cfl") {
            if (argc < 6) die("cfl needs <in.bin> <steps> <out.bin>");
            setup(sim, true);
            sim->setAdaptiveTimestep(true);
            for (int s = 0; s < std::atoi(argv[4]); ++s) sim->update();
            dump(argv[5], sim, 0, bi, vbi);
        } else {
            if (argc < 8) die("resume needs <in.bin> <steps_a> <steps_b> <ckpt> <out.bin>");
            setup(sim, true);
            for (int s = 0; s < std::atoi(argv[4]); ++s) sim->update();
            if (!sim->saveState(argv[6])) die("saveState failed");
            Nereus::SPH *again = iisph ? (Nereus::SPH *)new Nereus::IISPH() : new Nereus::SPH();
            again->_initialize();
            if (!again->loadState(argv[6])) die("loadState failed");
            setup(again, false);
            for (int s = 0; s < std::atoi(argv[5]); ++s) again->update();
            if (iisph) iters = static_cast<Nereus::IISPH *>(again)->getLastIterations();
            dump(argv[7], again, iters, bi, vbi);
            delete again;
        }
    } else if (mode == "mainscene") {
        if (argc < 5) die("mainscene needs <steps> <out.bin>");
        sim->generateParticleCube(make_SVec4(-0.4f, 0.04f, 0.5f, 1.f), make_SVec4(0.5f, 0.5f, 0.5f, 1.f), make_SVec4(0, 0, 0, 0));
        if (std::getenv("NEREUS_MAIN_GRAVITY_OFF")) sim->setGravity(0.0); // main.cpp:538
        sample_spheres::ss::sampleBox(bi, make_SVec3(-1, -1, -1), make_SVec3(3.f, 3.f, 3.f), 0.02);
        sample_spheres::boundary_forces::getVbi(vbi, bi, sim->getInteractionRadius());
        sim->setNumBoundaries(bi.size());
        sim->setBi((SReal *)bi.data());
        sim->setVbi(vbi.data());
        sim->updateGpuBoundaries(bi.size());
        const int steps = std::atoi(argv[3]);
        for (int s = 0; s < steps; ++s) sim->update();
        if (iisph) iters = static_cast<Nereus::IISPH *>(sim)->getLastIterations();
        dump(argv[4], sim, iters, bi, vbi);
    } else if (mode == "piston") {
        if (argc < 5) die("piston needs <steps> <out.bin>");
        sim->generateParticleCube(make_SVec4(-0.4f, 0.04f, 0.5f, 1.f), make_SVec4(0.5f, 0.5f, 0.5f, 1.f), make_SVec4(0, 0, 0, 0));
        sample_spheres::ss::sampleBox(bi, make_SVec3(-1, -1, -1), make_SVec3(3.f, 3.f, 3.f), 0.02);
        sample_spheres::boundary_forces::getVbi(vbi, bi, sim->getInteractionRadius());
        std::vector<SVec4> plate;
        for (int iy = 0; iy < 16; ++iy)
            for (int iz = 0; iz < 16; ++iz) plate.push_back(make_SVec4(-0.70f, -0.26f + 0.04f * iy, 0.20f + 0.04f * iz, 1.f));
        std::vector<SReal> plateVbi;
        sample_spheres::boundary_forces::getVbi(plateVbi, plate, sim->getInteractionRadius());
        std::vector<SUint> bodyOf(bi.size(), 0u);
        bodyOf.insert(bodyOf.end(), plate.size(), 1u);
        bi.insert(bi.end(), plate.begin(), plate.end());
        vbi.insert(vbi.end(), plateVbi.begin(), plateVbi.end());
        sim->setNumBoundaries(bi.size());
        sim->setBi((SReal *)bi.data());
        sim->setVbi(vbi.data());
        sim->updateGpuBoundaries(bi.size());
        sim->setBoundaryBodies(bodyOf.data(), 2);
        const double v[3] = {1.0, 0.0, 0.0}, w[3] = {0.0, 0.0, 0.0};
        sim->setBodyVelocity(1, v, w);
        const int steps = std::atoi(argv[3]);
        for (int s = 0; s < steps; ++s) sim->update();
        double x[3], q[4];
        sim->getBodyPose(1, x, q);
        std::printf("piston: plate origin x = %.9g after %d steps\n", x[0], steps);
        dump(argv[4], sim, 0, bi, vbi);
    } else {
        die("unknown mode");
    }
    sim->_finalize();
    delete sim;
    return 0;
}

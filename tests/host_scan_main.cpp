// host_scan_main.cpp — stand-alone driver of the scan geometry's HIP-free header (nrs_host_scan.h) for tests/test_host_scan_cpu.py:
// one command per line on stdin, one answer per line on stdout.  Reals travel as C99 hex floats (or nan / inf), integers as decimals.
// Built by the test with the host compiler, plain and under the sanitizers.  PREC is 32 or 64: the context's SReal.
//   thr PREC ir                                       -> thr LENLTIR R2LEH2
//   quant PREC gx gy gz origin(3) cellSize(3) ir      -> quant s(3) o(3) QT OK
//   win PREC gx gy gz WINW WINBASE                    -> win NUMBODIES gx gy gz NUMCELLS RESTSAME   (RESTSAME: no other byte of the parameters changed)
//   pow2 v | pow2grid a b c | wallblocks n            -> v V
//   superset PREC FILE N ir cellSize origin(3)        -> superset HITS MISSED FAR QT OK
//       FILE: N points, three float32 each.  Every pair (i, j): exact = dot(d, d) < r2LeH2 as the kernels form it (differences and the
//       dot product in SReal, rounded to float); kept = quant_dist2(guarded word of i, word of j) < qT.  HITS: exact pairs; MISSED: exact
//       pairs that are not kept; FAR: owners with quanta_far.
//   fprate PREC FILE N ir cellSize origin(3)          -> fprate EXACT KEPT
//       every 7th owner: EXACT = pairs with |d|^2 < ir^2 in double; KEPT = pairs kept by the integer test that are less than 2 ir apart on every axis
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "nereus_hip.h"
#include "nrs_host_scan.h"

using namespace nrs;

static double num(std::istringstream &in)
{
    std::string t;
    in >> t;
    return strtod(t.c_str(), nullptr);
}
static long long i64(std::istringstream &in)
{
    std::string t;
    in >> t;
    return strtoll(t.c_str(), nullptr, 10);
}

template <typename PARAMS> static PARAMS grid_params(std::istringstream &in)
{
    PARAMS P;
    std::memset(&P, 0, sizeof(P));
    for (int a = 0; a < 3; ++a) P.gridSize[a] = (uint32_t)i64(in);
    P.numCells = P.gridSize[0] * P.gridSize[1] * P.gridSize[2];
    return P;
}

template <typename PARAMS> static void cmd_quant(std::istringstream &in)
{
    typedef decltype(PARAMS::interactionRadius) R;
    PARAMS P = grid_params<PARAMS>(in);
    for (int a = 0; a < 3; ++a) P.worldOrigin[a] = (R)num(in);
    for (int a = 0; a < 3; ++a) P.cellSize[a] = (R)num(in);
    P.interactionRadius = (R)num(in);
    const ScanQuant q = scan_quant(P);
    printf("quant %a %a %a %a %a %a %u %d\n", (double)q.qc.s[0], (double)q.qc.s[1], (double)q.qc.s[2], q.qc.o[0], q.qc.o[1], q.qc.o[2], q.qT, (int)q.ok);
}

template <typename PARAMS> static void cmd_win(std::istringstream &in)
{
    PARAMS PU;
    unsigned char *b = reinterpret_cast<unsigned char *>(&PU);
    for (size_t k = 0; k < sizeof(PU); ++k) b[k] = (unsigned char)(37u + 11u * k); // every field holds something
    for (int a = 0; a < 3; ++a) PU.gridSize[a] = (uint32_t)i64(in);
    PU.numCells = PU.gridSize[0] * PU.gridSize[1] * PU.gridSize[2];
    const uint32_t winW = (uint32_t)i64(in);
    const int winBase = (int)i64(in);
    const PARAMS P = window_params(PU, winW, winBase);
    PARAMS back = P;
    back.numBodies = PU.numBodies; back.gridSize[0] = PU.gridSize[0]; back.numCells = PU.numCells;
    printf("win %u %u %u %u %u %d\n", P.numBodies, P.gridSize[0], P.gridSize[1], P.gridSize[2], P.numCells, (int)(std::memcmp(&back, &PU, sizeof(PU)) == 0));
}

template <typename PARAMS> struct Scene {
    typedef decltype(PARAMS::interactionRadius) R;
    std::vector<R> pos; // three per point
    std::vector<qword_t> word;
    std::vector<bool> far;
    size_t n = 0;
    ScanGeometry geo;
    R ir;
    bool read(std::istringstream &in)
    {
        std::string file;
        in >> file;
        n = (size_t)i64(in);
        PARAMS P;
        std::memset(&P, 0, sizeof(P));
        P.gridSize[0] = P.gridSize[1] = P.gridSize[2] = 8u;
        P.numCells = 512u;
        ir = P.interactionRadius = (R)num(in);
        P.cellSize[0] = P.cellSize[1] = P.cellSize[2] = (R)num(in);
        for (int a = 0; a < 3; ++a) P.worldOrigin[a] = (R)num(in);
        geo = scan_geometry(P);
        std::vector<float> raw(3 * n);
        FILE *f = fopen(file.c_str(), "rb");
        if (!f) return false;
        const size_t got = fread(raw.data(), sizeof(float), raw.size(), f);
        fclose(f);
        if (got != raw.size()) return false;
        pos.assign(raw.begin(), raw.end());
        word.resize(n);
        far.resize(n);
        const QuantCfg &q = geo.q.qc;
        for (size_t i = 0; i < n; ++i) {
            float t[3];
            for (int a = 0; a < 3; ++a) t[a] = quantize_axis<R>(pos[3 * i + a], q.o[a], q.s[a]);
            far[i] = quanta_far(t[0], t[1], t[2]);
            word[i] = far[i] ? 0u : pack_quanta(t[0], t[1], t[2]);
        }
        return true;
    }
    bool kept(size_t i, size_t j) const { return quant_dist2(word[i] | QP_GUARD, word[j]) < geo.q.qT; }
};

template <typename PARAMS> static void cmd_superset(std::istringstream &in)
{
    typedef decltype(PARAMS::interactionRadius) R;
    Scene<PARAMS> s;
    if (!s.read(in)) { printf("superset unreadable\n"); return; }
    unsigned long long hits = 0, missed = 0, far = 0;
    for (size_t i = 0; i < s.n; ++i) {
        far += s.far[i] ? 1u : 0u;
        for (size_t j = 0; j < s.n; ++j) {
            const R dx = s.pos[3 * i] - s.pos[3 * j], dy = s.pos[3 * i + 1] - s.pos[3 * j + 1], dz = s.pos[3 * i + 2] - s.pos[3 * j + 2];
            const float d2 = (float)(dx * dx + dy * dy + dz * dz); // dot(), nrs_math.h
            const bool exact = d2 < s.geo.thr.r2LeH2;
            hits += exact ? 1u : 0u;
            missed += (exact && !s.kept(i, j)) ? 1u : 0u;
        }
    }
    printf("superset %llu %llu %llu %u %d\n", hits, missed, far, s.geo.q.qT, (int)s.geo.q.ok);
}

template <typename PARAMS> static void cmd_fprate(std::istringstream &in)
{
    Scene<PARAMS> s;
    if (!s.read(in)) { printf("fprate unreadable\n"); return; }
    const double h = (double)s.ir;
    unsigned long long exact = 0, keptN = 0;
    for (size_t i = 0; i < s.n; i += 7)
        for (size_t j = 0; j < s.n; ++j) {
            double d[3], d2 = 0.0;
            bool near = true;
            for (int a = 0; a < 3; ++a) {
                d[a] = (double)s.pos[3 * i + a] - (double)s.pos[3 * j + a];
                d2 += d[a] * d[a];
                near = near && std::fabs(d[a]) < 2.0 * h;
            }
            exact += d2 < h * h ? 1u : 0u;
            keptN += (near && s.kept(i, j)) ? 1u : 0u;
        }
    printf("fprate %llu %llu\n", exact, keptN);
}

int main()
{
    std::string ln;
    while (std::getline(std::cin, ln)) {
        std::istringstream in(ln);
        std::string cmd;
        in >> cmd;
        if (cmd == "pow2") { printf("v %d\n", (int)is_pow2((uint32_t)i64(in))); continue; }
        if (cmd == "wallblocks") { printf("v %u\n", wall_blocks((uint32_t)i64(in))); continue; }
        if (cmd == "pow2grid") {
            uint32_t g[3];
            for (int a = 0; a < 3; ++a) g[a] = (uint32_t)i64(in);
            printf("v %d\n", (int)pow2_grid(g));
            continue;
        }
        const bool f64 = i64(in) == 64;
        if (cmd == "thr") {
            const double ir = num(in);
            const CutThresholds t = f64 ? make_thresholds<double>(ir) : make_thresholds<float>((float)ir);
            printf("thr %a %a\n", (double)t.lenLtIr, (double)t.r2LeH2);
        } else if (cmd == "quant") {
            if (f64) cmd_quant<nrs_params_f64>(in); else cmd_quant<nrs_params_f32>(in);
        } else if (cmd == "win") {
            if (f64) cmd_win<nrs_params_f64>(in); else cmd_win<nrs_params_f32>(in);
        } else if (cmd == "superset") {
            if (f64) cmd_superset<nrs_params_f64>(in); else cmd_superset<nrs_params_f32>(in);
        } else if (cmd == "fprate") {
            if (f64) cmd_fprate<nrs_params_f64>(in); else cmd_fprate<nrs_params_f32>(in);
        } else {
            printf("unknown %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}

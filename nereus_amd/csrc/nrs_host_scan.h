// nrs_host_scan.h — the geometry of the neighbour scan: the numbers the host prepares and the scan is exact by.  No HIP: the context
// (nrs_ctx_impl.h, derive_kernel_params) and a stand-alone host program (tests/host_scan_main.cpp) compile the same text, and the
// device reaches the quantiser through the vector forms of nrs_math.h and Sweep::scan_compact (nrs_kernels_tiled.h).
//   * the cell-table window that turns the caller's parameters into the kernels' (window_params);
//   * the two float cut-offs of the exact test (CutThresholds, make_thresholds);
//   * the quantisation set-up of the compact scan (ScanQuant, scan_quant) and the quantiser itself (quantize_axis, pack_quanta,
//     quanta_far, quant_delta);
//   * the small host rules of a launch: the power-of-two test of the grid and the wall workgroups of a gather launch.
// One wrong ulp in a cut-off or in the set-up drops a neighbour silently; DESIGN.md "scan geometry" has the tests and their mutations.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <math.h>

// a function the host and the device both call (next to nrs_math.h's NRS_DEV); a plain inline function for a host compiler
#ifdef __HIPCC__
#define NRS_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define NRS_HD inline
#endif

namespace nrs {

// ---- the cell-table window ------------------------------------------------------------------------------------------------------------
// P from PU (any struct with SphSimParams' field names): numBodies = first column of the window (0 = whole grid) and, where the slab
// exchange keeps a window narrower than the grid, gridSize[0] / numCells of that window.  Nothing else changes.
template <typename PARAMS> static inline PARAMS window_params(const PARAMS &PU, uint32_t winW, int winBase)
{
    PARAMS P = PU;
    P.numBodies = 0;
    if (winW && winW < PU.gridSize[0]) {
        P.numBodies = (uint32_t)winBase;
        P.gridSize[0] = winW;
        P.numCells = winW * PU.gridSize[1] * PU.gridSize[2];
    }
    return P;
}

// ---- the small host rules ---------------------------------------------------------------------------------------------------------------
static inline bool is_pow2(uint32_t v) { return v && !(v & (v - 1)); }
static inline bool pow2_grid(const uint32_t gridSize[3]) { return is_pow2(gridSize[0]) && is_pow2(gridSize[1]) && is_pow2(gridSize[2]); }
// wall workgroups of a gather launch (grid-stride over the wall list, whose length is only known on the device)
static inline uint32_t wall_blocks(uint32_t interiorBlocks) { return std::min<uint32_t>(1024u, std::max<uint32_t>(1u, interiorBlocks / 16u)); }

// ---- the cut-offs of the exact test -----------------------------------------------------------------------------------------------------
// Thresholds that turn the reference's two cut-off predicates into one float compare on the float dot
// product d2 = dot(r,r)  (exact: sqrtf and the products are monotone, correctly rounded):
//   lenLtIr : smallest float T with  sqrtf(T) >= ir          ⇒  (length(r) <  ir)        ⇔ d2 < T
//   r2LeH2  : smallest float T with  fl(sqrtf(T)^2) > h*h    ⇒  !(length(r)^2 > h^2)     ⇔ d2 < T
struct CutThresholds { float lenLtIr, r2LeH2; };
// the search (IEEE float arithmetic on the host), from (float)(ir * ir) downwards, then upwards.  R is the context's SReal.
template <typename R> static inline CutThresholds make_thresholds(R ir)
{
    CutThresholds t;
    {
        float T = (float)(ir * ir);
        auto ge = [&](float x) { return !((R)sqrtf(x) < ir); }; // NOT (length < ir)
        while (ge(T) && T > 0.0f) T = nextafterf(T, 0.0f);
        while (!ge(T)) T = nextafterf(T, INFINITY);
        t.lenLtIr = T;
    }
    {
        const R h2 = ir * ir;
        float T = (float)h2;
        auto gt = [&](float x) { float l = sqrtf(x); R r2 = l * l; return r2 > h2; };
        while (gt(T) && T > 0.0f) T = nextafterf(T, 0.0f);
        while (!gt(T)) T = nextafterf(T, INFINITY);
        t.r2LeH2 = T;
    }
    return t;
}

// ---- compact scan candidates (the neighbour scan of the interior workgroups, nrs_kernels_tiled.h) -----------------------------
// A quantised copy of every sorted position, written by the reorder kernels next to the exact one: the position modulo FOUR
// cells per axis.  Differences of such coordinates wrap, so for two particles less than two cells apart on every axis — which
// every pair inside the interaction radius is (scan_quant: h < ~2 cellSize, else the context does not use the compact scan) —
// the wrapped difference IS the coordinate difference in quanta, whatever cells the two sit in.  The scan keeps a candidate when
// the integer squared distance is below (h / quantum + QP_MARGIN)^2: a SUPERSET of the exact hits; the process phase applies the
// exact float test to the exact position, which it has to gather anyway, and compacts the list before it is published.
struct QuantCfg { double o[3]; float s[3]; }; // grid origin, quanta per metre (QP_PER_CELL / cellSize)
// 4-byte quantised candidates: measured faster than a 16-bit-per-axis form and than exact positions, DESIGN.md §4 (what a candidate
// costs is its bytes through the L1 path and its register, not the distance arithmetic).
// 10 bits per axis at bits 0 / 11 / 22 (units of cellSize/256, modulo 4 cells); bits 10 and 21 are guard bits, left 0.  With the
// guard bits SET in the owner's word, ONE 32-bit subtraction gives the three differences modulo 1024 (each guard absorbs its
// field's borrow); three sign extensions, three 24-bit multiplies and an add give the squared distance (about 3 % false positives).
typedef uint32_t qword_t;
constexpr uint32_t QP_GUARD = (1u << 10) | (1u << 21);
constexpr float QP_PER_CELL = 256.0f;
// |k_i - k_j - (t_i - t_j)| < 1 (two floors) + 2 * 0.19 (relative error <= 3 * 2^-24 on |t| < 2^20 + 2^9) per axis, so
// |dk| <= |dt| + 1.38 * sqrt(3) = |dt| + 2.39; + the float rounding of the exact test itself
constexpr float QP_MARGIN = 2.5f;
constexpr float QP_FAR = 1048576.0f; // 2^20 quanta = 4096 cells from the grid origin: an owner beyond that (or with a NaN coordinate) is scanned on exact positions (quanta_far)
constexpr float QP_HALF = 511.0f;

// one coordinate in quanta from the grid origin (R: the precision of the position)
template <typename R> NRS_HD float quantize_axis(R p, double o, float s) { return (float)(p - (R)o) * s; }
NRS_HD qword_t pack_quanta(float tx, float ty, float tz)
{
    const uint32_t kx = (uint32_t)(int)floorf(tx) & 1023u, ky = (uint32_t)(int)floorf(ty) & 1023u, kz = (uint32_t)(int)floorf(tz) & 1023u;
    return kx | (ky << 11) | (kz << 22);
}
// A coordinate the error budget of the quanta covers (false for NaN).  An owner with a coordinate that fails this is too far from
// the grid origin and is scanned on exact positions: quanta_far here, quant_far (nrs_math.h) and Sweep::scan_compact on the device,
// which each state the conjunction over the three axes themselves (one shared three-argument form made the reorder kernels'
// instructions differ, DESIGN.md "scan geometry").
NRS_HD bool quanta_near(float t) { return fabsf(t) < QP_FAR; }
static inline bool quanta_far(float tx, float ty, float tz) { return !(quanta_near(tx) && quanta_near(ty) && quanta_near(tz)); }
// the three wrapped differences of an owner's GUARDED word Qi = pack_quanta(..) | QP_GUARD and a candidate's word c:
// one subtraction, three sign extensions
struct QuantDelta { int x, y, z; };
NRS_HD QuantDelta quant_delta(uint32_t Qi, uint32_t c)
{
    const uint32_t t = Qi - c;
    QuantDelta d;
    d.x = ((int)(t << 22)) >> 22; d.y = ((int)(t << 11)) >> 22; d.z = ((int)t) >> 22;
    return d;
}
// ... and their sum of squares, which the scan compares with qT.  (The device forms the same integer with two v_mad_i32_i24 and a
// 24-bit multiply, Sweep::scan_compact: |d| <= 512, every product and the sum are exact either way.)
static inline uint32_t quant_dist2(uint32_t Qi, uint32_t c)
{
    const QuantDelta d = quant_delta(Qi, c);
    return (uint32_t)(d.z * d.z + (d.y * d.y + d.x * d.x));
}

// The set-up: quanta per metre, the threshold qT of the superset test, and whether the geometry allows the compact scan at all (a pair
// inside the interaction radius must be less than two cells apart on every axis).  P: the KERNELS' parameters (window_params).
struct ScanQuant { QuantCfg qc; uint32_t qT; bool ok; };
template <typename PARAMS> static inline ScanQuant scan_quant(const PARAMS &P)
{
    typedef decltype(PARAMS::interactionRadius) R;
    ScanQuant q;
    float hq = 0.0f;
    q.ok = P.gridSize[0] >= 4u; // (narrower grids alias the row's three cells: tags by position fail)
    for (int a = 0; a < 3; ++a) {
        q.qc.o[a] = (double)P.worldOrigin[a];
        q.qc.s[a] = QP_PER_CELL / (float)P.cellSize[a];
        const float r = (float)P.interactionRadius * q.qc.s[a];
        q.ok = q.ok && P.cellSize[a] > (R)0 && std::isfinite(q.qc.s[a]) && (r + QP_MARGIN < QP_HALF);
        hq = std::max(hq, r);
    }
    const double lim = (double)hq + (double)QP_MARGIN;
    q.qT = q.ok ? (uint32_t)std::ceil(lim * lim) + 1u : 0u;
    return q;
}

// what the context keeps, recomputed whenever its parameters or its window change
struct ScanGeometry { ScanQuant q; CutThresholds thr; };
template <typename PARAMS> static inline ScanGeometry scan_geometry(const PARAMS &P)
{
    return ScanGeometry{scan_quant(P), make_thresholds(P.interactionRadius)};
}

} // namespace nrs

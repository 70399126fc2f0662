// nrs_math.h — device-side vector layer and smoothing kernels for the gfx950 SPH step.
//
// Semantics to match (not code): the reference's helper_math.h overload set
// (common/cuda_helpers/helper_math.h:817-829, 1000-1008, 1251-1301) takes and returns *float* scalars
// even when SVec3 is double3, and common/kernels_impl.cuh:85-203 mixes pow/powf.
// All arithmetic is IEEE (this file is compiled with -ffp-contract=off; division and sqrt are the
// correctly rounded forms), so the fp32 path can be compared bit-for-bit with the CPU oracle.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define NRS_DEV __device__ __forceinline__
#include "nrs_host_scan.h" // NRS_HD; the scan's geometry and its quantiser, one definition for the host and the device

namespace nrs {

template <typename R> struct V3 { R x, y, z; };

template <typename R> struct Vec4T;
template <> struct Vec4T<float> { typedef float4 type; };
template <> struct Vec4T<double> { typedef double4 type; };

template <typename R> NRS_DEV V3<R> mk3(R x, R y, R z) { V3<R> v; v.x = x; v.y = y; v.z = z; return v; }
template <typename R, typename T4> NRS_DEV V3<R> xyz(const T4 &a) { return mk3<R>(a.x, a.y, a.z); }
template <typename R> NRS_DEV typename Vec4T<R>::type mk4(R x, R y, R z, R w)
{
    typename Vec4T<R>::type v; v.x = x; v.y = y; v.z = z; v.w = w; return v;
}
template <typename R> NRS_DEV typename Vec4T<R>::type mk4(V3<R> a, R w) { return mk4<R>(a.x, a.y, a.z, w); }

template <typename R> NRS_DEV V3<R> operator+(V3<R> a, V3<R> b) { return mk3<R>(a.x + b.x, a.y + b.y, a.z + b.z); }
template <typename R> NRS_DEV V3<R> operator-(V3<R> a, V3<R> b) { return mk3<R>(a.x - b.x, a.y - b.y, a.z - b.z); }
// scalar operands are float by signature, as in the reference
template <typename R> NRS_DEV V3<R> operator*(V3<R> a, float b) { return mk3<R>(a.x * b, a.y * b, a.z * b); }
template <typename R> NRS_DEV V3<R> operator*(float b, V3<R> a) { return mk3<R>(b * a.x, b * a.y, b * a.z); }
template <typename R> NRS_DEV V3<R> operator/(V3<R> a, float b) { return mk3<R>(a.x / b, a.y / b, a.z / b); }
template <typename R> NRS_DEV float dot(V3<R> a, V3<R> b) { return (float)(a.x * b.x + a.y * b.y + a.z * b.z); }
// NB: __fsqrt_rn is the NATIVE (1-ulp) sqrt in this HIP; sqrtf is the correctly rounded one (hipcc default
// -fhip-fp32-correctly-rounded-divide-sqrt).
NRS_DEV float sqrt_rn(float x) { return sqrtf(x); }
template <typename R> NRS_DEV float length(V3<R> v) { return sqrt_rn(dot(v, v)); }

// ---- divisions and square roots for operands in range --------------------------------------------------------------------------------
// The compiler expands a correctly rounded fp32 division into v_div_scale x2, v_rcp, fma, fma, mul, fma, fma, fma, v_div_fmas, v_div_fixup
// (AMDGPU LowerFDIV32; the ISA of `a / b` on gfx950 is exactly that, 11 instructions) and sqrtf into a scaling select, v_sqrt, two integer
// neighbours, two residual fmas, two selects, the unscaling and a class test (15).  The scaling exists for operands near the ends of the
// exponent range: v_div_scale returns its operand UNCHANGED (and clears the flag v_div_fmas reads, which then is a plain fma) when numerator
// and denominator are non-zero, the denominator and its reciprocal are normal, the numerator is not tiny, the quotient is not denormal and
// the exponents are less than 96 apart; v_div_fixup then only re-applies the quotient's sign.  For such operands the eight arithmetic steps
// in between ARE the division, bit for bit — nothing is approximated, the scaling is simply not needed — and divisions by the same
// denominator share the first three steps (for a launch constant they are formed once per thread).  Likewise sqrtf without its scaling for
// 2^-96 <= x < inf.
// The region the forms are used in (every use states the guard that puts its operands there, and what runs when the guard fails — the plain
// `/` and sqrtf):  numerator +0, or 2^-90 <= |n| <= 2^90 with 2^-90 <= |d| <= 2^90 and 2^-104 < |n / d| < 2^96.
// Why 2^-90 and not the ISA manual's "biased exponent above 23" (2^-103): the residual n - d q of a quotient step is a multiple of
// 2^(e_n - 47); it is a float — and the step exact — only while that is at least 2^-149.  tools/check_div2.hip found the case: for d = 2e-4
// the numerators +-1.34756e-31 (biased exponent 24) are a last-bit tie that the bare steps round the other way.  The same tool compares the
// forms with `/` and sqrtf on the device over the region: all 2^32 numerator patterns for twelve denominators, 2^32 random pairs, and every
// float in [2^-96, inf) for the square root — 0 differences.
NRS_DEV float rcp_refined(float d) // steps 1-3: the reciprocal every quotient by d is built from
{
    const float r = __builtin_amdgcn_rcpf(d);
    return __builtin_fmaf(__builtin_fmaf(-d, r, 1.0f), r, r);
}
NRS_DEV float div_steps(float n, float d, float y) // steps 4-8, y = rcp_refined(d)
{
    const float q0 = n * y;
    const float q1 = __builtin_fmaf(__builtin_fmaf(-d, q0, n), y, q0);
    return __builtin_fmaf(__builtin_fmaf(-d, q1, n), y, q1);
}
NRS_DEV float sqrt_inrange(float x) // 2^-96 <= x < inf
{
    const float s = __builtin_amdgcn_sqrtf(x);
    const float dn = __uint_as_float(__float_as_uint(s) - 1u), up = __uint_as_float(__float_as_uint(s) + 1u);
    const float vp = __builtin_fmaf(-dn, s, x), vs = __builtin_fmaf(-up, s, x);
    float o = 0.f >= vp ? dn : s;
    o = 0.f < vs ? up : o;
    return o;
}

// two floats per lane on packed fp32 (v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32 round each component like the scalar forms): the pairs of
// the force walk (two hits) and of the density walk (two list entries), and the in-range steps above for both components at once
typedef float f2 __attribute__((ext_vector_type(2)));
struct V3x2 { f2 x, y, z; };
NRS_DEV f2 splat2(float v) { f2 r = {v, v}; return r; }
NRS_DEV f2 pair2(float a, float b) { f2 r = {a, b}; return r; }
NRS_DEV f2 dot2(const V3x2 &a, const V3x2 &b) { return a.x * b.x + a.y * b.y + a.z * b.z; } // ((x + y) + z), as dot()
NRS_DEV f2 fma2(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
NRS_DEV f2 rcp_refined2(f2 d) // steps 1-3: the reciprocal every quotient by d is built from
{
    const f2 r = pair2(__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y));
    return fma2(fma2(-d, r, splat2(1.0f)), r, r);
}
NRS_DEV f2 div_steps2(f2 n, f2 d, f2 y) // steps 4-8
{
    const f2 nd = -d;
    const f2 q0 = n * y;
    const f2 q1 = fma2(fma2(nd, q0, n), y, q0);
    return fma2(fma2(nd, q1, n), y, q1);
}
NRS_DEV f2 sqrt_inrange2(f2 x)
{
    const float sa = __builtin_amdgcn_sqrtf(x.x), sb = __builtin_amdgcn_sqrtf(x.y);
    const f2 s = pair2(sa, sb);
    const f2 dn = pair2(__uint_as_float(__float_as_uint(sa) - 1u), __uint_as_float(__float_as_uint(sb) - 1u));
    const f2 up = pair2(__uint_as_float(__float_as_uint(sa) + 1u), __uint_as_float(__float_as_uint(sb) + 1u));
    const f2 vp = fma2(-dn, s, x), vs = fma2(-up, s, x);
    f2 o = s;
    o.x = 0.f >= vp.x ? dn.x : o.x; o.x = 0.f < vs.x ? up.x : o.x;
    o.y = 0.f >= vp.y ? dn.y : o.y; o.y = 0.f < vs.y ? up.y : o.y;
    return o;
}

// x^3 the way g++ evaluates pow(SReal,int): in double, rounded once to SReal (kernels_impl.cuh:95)
template <typename R> NRS_DEV R cube_via_double(R x) { double d = (double)x; return (R)(d * d * d); }
// powf(x,2) (kernels_impl.cuh:113): float square, also in fp64 builds
template <typename R> NRS_DEV R square_via_float(R x) { float f = (float)x; return (R)(f * f); }
// powf(x,7) (sph_kernel_impl.cuh:426): float result of x^7; computed in double and rounded once
NRS_DEV float pow7f(float x)
{
    double d = (double)x, d2 = d * d, d4 = d2 * d2;
    return (float)(d4 * d2 * d);
}

enum { KS_MONAGHAN = 0, KS_MULLER = 1 };

// Muller poly6 W (kernels_impl.cuh:85-98)
template <typename R> NRS_DEV R Wdefault(V3<R> r, R h, R kpoly)
{
    R r2 = length(r) * length(r);
    R h2 = h * h;
    if (r2 > h2) return (R)0.0;
    R b = cube_via_double<R>(h2 - r2);
    return kpoly * b;
}
// gradient of poly6 (:103-116)
template <typename R> NRS_DEV V3<R> Wdefault_grad(V3<R> r, R h, R kpoly_grad)
{
    R r2 = length(r) * length(r);
    R h2 = h * h;
    if (r2 > h2) return mk3<R>(0, 0, 0);
    R b = square_via_float<R>(h2 - r2);
    return kpoly_grad * r * b;
}
// spiky gradient (:121-135)
template <typename R> NRS_DEV V3<R> Wpressure_grad(V3<R> r, R h, R kpress_grad)
{
    R rlen = length(r);
    R r2 = rlen * rlen;
    R h2 = h * h;
    if (r2 > h2) return mk3<R>(0, 0, 0);
    R c = (h - rlen) * (h - rlen);
    return kpress_grad * (r / rlen) * c;
}
// viscosity kernel "gradient" (:140-154)
template <typename R> NRS_DEV V3<R> Wviscosity_grad(V3<R> r, R h, R kvisc_grad, R kvisc_denum)
{
    R rlen = length(r);
    R r2 = rlen * rlen;
    R h2 = h * h;
    if (r2 > h2) return mk3<R>(0, 0, 0);
    R c = -(3 * rlen / kvisc_denum) + (2 / (h2)) - (h / (2 * rlen * rlen * rlen));
    return kvisc_grad * r * c;
}
// Monaghan cubic spline (:159-203); constants evaluated in double as the host compiler does
template <typename R> NRS_DEV R Wmonaghan(V3<R> r, R h)
{
    R value = (R)0.0;
    R invH = (R)(1.0 / h);
    R m_v = (R)(1.0 / (4.0 * 3.14159265358979323846 * h * h * h));
    R q = length(r) * invH;
    if (q >= 0 && q < 1)
        value = m_v * ((2 - q) * (2 - q) * (2 - q) - 4.0f * (1 - q) * (1 - q) * (1 - q));
    else if (q >= 1 && q < 2)
        value = m_v * ((2 - q) * (2 - q) * (2 - q));
    else
        value = 0.0f;
    return value;
}
template <typename R> NRS_DEV V3<R> Wmonaghan_grad(V3<R> r, R h)
{
    R m_g = (R)(1.0 / (4.0 * 3.14159265358979323846 * h * h * h));
    R dist = length(r);
    R invH = (R)(1.0 / h);
    R q = dist * invH;
    V3<R> gradient = mk3<R>(0, 0, 0);
    if (q >= 0 && q < 1) {
        R scalar = -3.0f * (2 - q) * (2 - q);
        scalar += 12.0f * (1 - q) * (1 - q);
        gradient = (m_g * invH * scalar / dist) * r;
    } else if (q >= 1 && q < 2) {
        R scalar = -3.0f * (2 - q) * (2 - q);
        gradient = (m_g * scalar * invH / dist) * r;
    }
    return gradient;
}

// Akinci cohesion kernel (:208-228): the reference's expression in its operand types (2.0 * len is a double product)
template <typename R> NRS_DEV R Cakinci(V3<R> r, R h, R ksurf1, R ksurf2)
{
    R len = length(r);
    R poly = ksurf1;
    R hr = h - len;
    if (2.0 * len > h && len <= h) {
        R a = (hr * hr * hr) * (len * len * len);
        return poly * a;
    } else if (len > 0.0 && 2 * len <= h) {
        R a = 2 * (hr * hr * hr) * (len * len * len);
        R b = ksurf2;
        return poly * (a - b);
    }
    return (R)0.0;
}
// the radicand -4 r^2 / h + 6 r - 2 h of the adhesion kernel (:238-239): b is formed in double and rounded to SReal
template <typename R> NRS_DEV R Aboundary_radicand(R rl, R h)
{
    R a = -((4 * (rl * rl)) / (h));
    R b = (R)(6.0 * rl - 2.0 * h);
    return a + b;
}
// Akinci adhesion kernel (:233-247): powf on a float, also in the fp64 build; NaN where roundoff leaves the radicand below zero
// (next to r = h / 2 and r = h), as the reference
template <typename R> NRS_DEV R Aboundary(V3<R> r, R h, R bpol)
{
    R rl = length(r);
    if (2.0 * rl > h && rl <= h) {
        R res = powf((float)Aboundary_radicand<R>(rl, h), (float)(1.0 / 4.0));
        return bpol * res;
    }
    return (R)0.0;
}
// ... as the force walk evaluates it (DESIGN.md "Akinci surface tension and adhesion"): the radicand clamped at 0, and the fourth
// root as two correctly rounded float square roots — within one float ulp of powf, and the same bits on every IEEE machine
template <typename R> NRS_DEV R Aboundary_clamped(V3<R> r, R h, R bpol)
{
    R rl = length(r);
    if (2.0 * rl > h && rl <= h) {
        const float rad = (float)Aboundary_radicand<R>(rl, h);
        R res = sqrt_rn(sqrt_rn(rad > 0.0f ? rad : 0.0f));
        return bpol * res;
    }
    return (R)0.0;
}

template <typename R, int KSET> NRS_DEV R W_dens(V3<R> r, R ir, R kp)
{
    if (KSET == KS_MULLER) return Wdefault<R>(r, ir, kp);
    return Wmonaghan<R>(r, ir);
}
template <typename R, int KSET> NRS_DEV V3<R> W_grad(V3<R> r, R ir, R kpg)
{
    if (KSET == KS_MULLER) return Wdefault_grad<R>(r, ir, kpg);
    return Wmonaghan_grad<R>(r, ir);
}
// length() and W_grad() for the hit-list walks of the IISPH chain (Muller kernels): the square root as the bare steps of the compiler's
// expansion ("operands in range" above; an argument below 2^-96 — coincident particles — takes sqrtf).  Same values, bit for bit: dot() and
// length() are float in both precisions, Wdefault_grad squares that float length.
NRS_DEV float length_listed(float d2)
{
    return d2 >= 0x1p-96f ? sqrt_inrange(d2) : sqrt_rn(d2);
}
template <typename R> NRS_DEV V3<R> Wdefault_grad_len(V3<R> r, float rlen, R h, R kpoly_grad) // Wdefault_grad with length(r) handed in
{
    R r2 = rlen * rlen;
    R h2 = h * h;
    if (r2 > h2) return mk3<R>(0, 0, 0);
    R b = square_via_float<R>(h2 - r2);
    return kpoly_grad * r * b;
}
template <typename R, int KSET> NRS_DEV V3<R> W_grad_listed(V3<R> r, R ir, R kpg)
{
    if constexpr (KSET == KS_MULLER) return Wdefault_grad_len<R>(r, length_listed(dot(r, r)), ir, kpg);
    else return W_grad<R, KSET>(r, ir, kpg);
}

// SphSimParams, byte-identical to nrs_params_f32 / nrs_params_f64 (include/nereus_hip.h)
template <typename R> struct Params {
    uint32_t gridSize[3];
    uint32_t numCells;
    R worldOrigin[3];
    R cellSize[3];
    uint32_t numBodies;
    uint32_t maxParticlesPerCell;
    R gasStiffness, viscosity, surfaceTension, restDensity, particleMass, interactionRadius, timestep, particleRadius;
    R gravity[3];
    R soundSpeed;
    R beta;
    R kpoly, kpoly_grad, kpress_grad, kvisc_grad, kvisc_denum, ksurf1, ksurf2, bpol;
};
static_assert(sizeof(Params<float>) == 132, "fp32 SphSimParams must be 132 bytes");
static_assert(sizeof(Params<double>) == 240, "fp64 SphSimParams must be 240 bytes");

struct I3 { int x, y, z; };

// calcGridPos (sph_kernel_impl.cuh:105-113): true division, then floor
template <typename R> NRS_DEV I3 calcGridPos(const Params<R> &P, V3<R> p)
{
    I3 g;
    g.x = (int)floor((p.x - P.worldOrigin[0]) / P.cellSize[0]);
    g.y = (int)floor((p.y - P.worldOrigin[1]) / P.cellSize[1]);
    g.z = (int)floor((p.z - P.worldOrigin[2]) / P.cellSize[2]);
    return g;
}
NRS_DEV uint32_t umul24(uint32_t a, uint32_t b) { return (a & 0xffffffu) * (b & 0xffffffu); }
// calcGridHash (:118-125): power-of-two wrap, 24-bit multiplies.
// P.numBodies (unused by the reference, common/sph_kernel.cuh:27) carries the first cell-x column of the context's cell-table
// WINDOW in the device-side copy of the parameters: 0 for a single domain (then this is the reference's hash exactly); a slab
// rank keeps tables only for its own columns + halo, gridSize[0] being the (power-of-two) window width (nrs_ctx_impl.h).
template <typename R> NRS_DEV uint32_t grid_x(const Params<R> &P, int gx) { return ((uint32_t)gx - P.numBodies) & (P.gridSize[0] - 1); }
template <typename R> NRS_DEV uint32_t calcGridHash(const Params<R> &P, int gx, int gy, int gz)
{
    uint32_t x = grid_x<R>(P, gx);
    uint32_t y = (uint32_t)gy & (P.gridSize[1] - 1);
    uint32_t z = (uint32_t)gz & (P.gridSize[2] - 1);
    return umul24(umul24(z, P.gridSize[1]), P.gridSize[0]) + umul24(y, P.gridSize[0]) + x;
}

static constexpr uint32_t CELL_EMPTY = 0xffffffffu;
constexpr int BLOCK = 256;
static inline uint32_t nblocks(uint64_t n) { return (uint32_t)((n + BLOCK - 1) / BLOCK); } // workgroups of BLOCK threads over n items

// ---- compact scan candidates (the neighbour scan of the interior workgroups, nrs_kernels_tiled.h) -----------------------------
// What a quantised position is, the QP_* constants and the arithmetic per coordinate: nrs_host_scan.h (included above; the host
// prepares QuantCfg and the scan's threshold from the same header).  Here: its forms on a V3.
template <typename R> NRS_DEV void quantize_t(const QuantCfg &q, V3<R> p, float &tx, float &ty, float &tz)
{
    tx = quantize_axis<R>(p.x, q.o[0], q.s[0]);
    ty = quantize_axis<R>(p.y, q.o[1], q.s[1]);
    tz = quantize_axis<R>(p.z, q.o[2], q.s[2]);
}
// an owner too far from the grid origin for the error budget of the quanta, or with a NaN coordinate
template <typename R> NRS_DEV bool quant_far(const QuantCfg &q, V3<R> p)
{
    float tx, ty, tz;
    quantize_t<R>(q, p, tx, ty, tz);
    return !(quanta_near(tx) && quanta_near(ty) && quanta_near(tz));
}
template <typename R> NRS_DEV qword_t quantize_pos(const QuantCfg &q, V3<R> p)
{
    float tx, ty, tz;
    quantize_t<R>(q, p, tx, ty, tz);
    return pack_quanta(tx, ty, tz);
}

} // namespace nrs

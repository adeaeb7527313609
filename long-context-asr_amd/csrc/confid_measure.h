// The frame measures of include/sconf_confid.h as device code: what confid.hip (one softmax per row) and calib.hip (K temperatures per
// row) share, so that the column of the sweep at temperature 1 is sconf_confid_frames bit for bit.  Include after common.h and
// sconf_confid.h, in a file built without fast-math.
#pragma once

namespace {

constexpr int QUADS = 4;                       // quads of four elements a lane of the register path holds at most
constexpr int ROW_CAPACITY = 64 * QUADS * 4;   // 1024 classes in the registers of one wave
constexpr int BLOCK = 256;
constexpr int BLOCK_CAPACITY = BLOCK * QUADS * 4; // 4096 classes in the registers of one workgroup
constexpr int NO_INDEX = 0x7fffffff;

// what the host works out once per call: no division by alpha - 1 and no logarithm of V on the device
struct Measure {
    int method, norm;
    float alpha;
    float V;            // classes
    float inv_vm1;      // 1 / (V - 1)
    float inv_lnv;      // 1 / ln V
    float inv_am1;      // 1 / (alpha - 1)                      (TSALLIS, RENYI)
    float inv_hmax;     // 1 / H_max of TSALLIS
    float e_hmax;       // e^-H_max of TSALLIS
    float inv_1me;      // 1 / (1 - e^-H_max)
};

struct Best { float v; int i; };
__device__ __forceinline__ void take(Best& b, float v, int i) { if (v > b.v || (v == b.v && i < b.i)) { b.v = v; b.i = i; } }
__device__ __forceinline__ Best wave_best(Best b) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(b.v, o, 64); const int oi = __shfl_xor(b.i, o, 64);
        take(b, ov, oi);
    }
    return b;
}

// e^d for d <= 0 on the hardware's 2^x: the rounding of d log2(e) moves e^d by |d| e^d 2^-24 at most, which is below 2^-25 for every
// d (the terms that carry a sum have small |d|), so the per-element exponential need not be the math library's
__device__ __forceinline__ float exp_(float d) { return __builtin_amdgcn_exp2f(d * 1.4426950408889634f); }

// the three sums of one element d = x - m <= 0 (or -inf): e^d, e^d d and e^(alpha d)
struct Sums { float z, t, a; };
template <int METHOD> __device__ __forceinline__ void add(Sums& s, float d, float alpha) {
    const float e = exp_(d);
    s.z += e;
    if (METHOD == SCONF_CONFID_SHANNON) s.t += e > 0.f ? e * d : 0.f;                  // (0 * -inf is no part of the sum)
    if (METHOD == SCONF_CONFID_TSALLIS || METHOD == SCONF_CONFID_RENYI) s.a += exp_(alpha * d);
}

template <int METHOD> __device__ __forceinline__ float confidence(const Sums& s, const Measure& q) {
    if (METHOD == SCONF_CONFID_MAX_PROB) return (q.V / s.z - 1.f) * q.inv_vm1;
    const float lnz = logf(s.z);
    float H;
    if (METHOD == SCONF_CONFID_SHANNON) H = lnz - s.t / s.z;
    else {
        const float ln_sa = logf(s.a) - q.alpha * lnz;
        if (METHOD == SCONF_CONFID_RENYI) H = -ln_sa * q.inv_am1;
        else {
            H = (1.f - expf(ln_sa)) * q.inv_am1;
            return q.norm == SCONF_CONFID_LIN ? 1.f - H * q.inv_hmax : (expf(-H) - q.e_hmax) * q.inv_1me;
        }
    }
    return q.norm == SCONF_CONFID_LIN ? 1.f - H * q.inv_lnv : (q.V * expf(-H) - 1.f) * q.inv_vm1;
}

// a quad of four neighbouring elements from column c on: one 16-byte load where the row allows it, single elements elsewhere;
// columns at and behind `classes` are never loaded and count as -inf
__device__ __forceinline__ void load_quad(const float* __restrict__ xr, int c, int C, int vec, float (&v)[4]) {
    if (vec && c + 4 <= C) load4(xr + c, v);
    else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = c + e < C ? xr[c + e] : -INFINITY;
    }
}

template <int G> __device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
template <int G> __device__ __forceinline__ Best group_best(Best b) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) {
        const float ov = __shfl_xor(b.v, o, 64); const int oi = __shfl_xor(b.i, o, 64);
        take(b, ov, oi);
    }
    return b;
}
template <int G> __device__ __forceinline__ bool group_any(bool f) {
    int v = f;
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
    return v != 0;
}

inline bool alpha_ok(float alpha) { return (alpha > 0.f && alpha < 1.f) || (alpha > 1.f && alpha <= 4.f); }

// the constants of a call, in double on the host and rounded once
inline Measure measure_of(int method, int norm, float alpha, int64_t classes) {
    const double V = (double)classes, lnv = log(V);
    Measure q{};
    q.method = method; q.norm = norm; q.alpha = alpha;
    q.V = (float)V; q.inv_vm1 = (float)(1.0 / (V - 1.0)); q.inv_lnv = (float)(1.0 / lnv);
    if (method == SCONF_CONFID_TSALLIS || method == SCONF_CONFID_RENYI) {
        const double am1 = (double)alpha - 1.0, hmax = (1.0 - exp(-am1 * lnv)) / am1;
        q.inv_am1 = (float)(1.0 / am1); q.inv_hmax = (float)(1.0 / hmax); q.e_hmax = (float)exp(-hmax); q.inv_1me = (float)(1.0 / (1.0 - exp(-hmax)));
    }
    return q;
}

}  // namespace

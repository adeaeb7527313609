// Shared device/host helpers for the sconf HIP library (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <stdlib.h>
#include <initializer_list>
#include "../../include/sconf.h"   // the public C ABI: every SCONF_API definition is compiled against its declaration

typedef __bf16 bf16;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;

#define SCONF_API extern "C" __attribute__((visibility("default")))
#include "gfx950.h"                // inline-asm, LDS-DMA, wait, tie and stamp primitives (needs the vector types above)

// ---- error reporting (C ABI: non-zero return + sconf_last_error()) ---------------------------
int sconf_set_error(const char* fmt, ...);
#define SCONF_REQUIRE(cond, ...) do { if (!(cond)) return sconf_set_error(__VA_ARGS__); } while (0)
#define SCONF_LAUNCH_OK(name) do { hipError_t e_ = hipGetLastError(); \
    if (e_ != hipSuccess) return sconf_set_error("%s: launch failed: %s", name, hipGetErrorString(e_)); } while (0)

// ---- library-private functions called across files (defined in subsample_mfma.hip, called from subsample.hip) --------
// conv0 on the matrix cores; the launchers return 1 when they took the problem
int sconf_stage01_fwd_mfma(const void* x, int x_dtype, const float* w0, const float* b0, const float* wd, const float* bd, void* d1,
                           int64_t B, int64_t F, int64_t T, int64_t C, hipStream_t stream);
int sconf_stage01_bwd_mfma(const void* dd1, const void* x, int x_dtype, const float* w0, const float* b0, const float* wd,
                           float* dw0, float* db0, float* dwd, float* dbd, void* workspace, int64_t workspace_bytes,
                           int64_t B, int64_t F, int64_t T, int64_t C, hipStream_t stream);
int sconf_dwconv_window_fwd(const void* x, const float* w, const float* bias, void* y, int64_t B, int64_t Ti, int64_t Fi, int64_t C, hipStream_t stream);
int64_t stage01_bwd_mfma_workspace(int64_t B, int64_t F, int64_t T, int64_t C);
int stage01_mfma_slabs(int64_t F, int64_t C, int bwd);

// ---- device helpers --------------------------------------------------------------------------
__device__ __forceinline__ float bf2f(bf16 x) { return (float)x; }
__device__ __forceinline__ bf16 f2bf(float x) { return (bf16)x; }   // v_cvt_pk_bf16_f32 (RNE, NaN-safe)

// a sample's length: v[b], or dflt where the caller passed no length vector
__device__ __forceinline__ int len_of(const int* v, int b, int dflt) { return v ? v[b] : dflt; }

template <typename T> __device__ __forceinline__ float ld_f(const T* p);
template <> __device__ __forceinline__ float ld_f<float>(const float* p) { return *p; }
template <> __device__ __forceinline__ float ld_f<bf16>(const bf16* p) { return (float)*p; }
template <typename T> __device__ __forceinline__ void st_f(T* p, float v);
template <> __device__ __forceinline__ void st_f<float>(float* p, float v) { *p = v; }
template <> __device__ __forceinline__ void st_f<bf16>(bf16* p, float v) { *p = (bf16)v; }

// 8-element vector load/store as floats (16 B for bf16, 2x16 B for f32)
__device__ __forceinline__ void load8(const bf16* p, float (&v)[8]) {
    bf16x8 t = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (float)t[i];
}
__device__ __forceinline__ void load8(const float* p, float (&v)[8]) {
    float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void store8(bf16* p, const float (&v)[8]) {
    bf16x8 t;
#pragma unroll
    for (int i = 0; i < 8; ++i) t[i] = (bf16)v[i];
    *reinterpret_cast<bf16x8*>(p) = t;
}
__device__ __forceinline__ void store8(float* p, const float (&v)[8]) {
    reinterpret_cast<float4*>(p)[0] = make_float4(v[0], v[1], v[2], v[3]);
    reinterpret_cast<float4*>(p)[1] = make_float4(v[4], v[5], v[6], v[7]);
}
__device__ __forceinline__ void load4(const bf16* p, float (&v)[4]) {
    bf16x4 t = *reinterpret_cast<const bf16x4*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (float)t[i];
}
__device__ __forceinline__ void load4(const float* p, float (&v)[4]) {
    float4 a = *reinterpret_cast<const float4*>(p);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
}
__device__ __forceinline__ void store4(bf16* p, const float (&v)[4]) {
    bf16x4 t;
#pragma unroll
    for (int i = 0; i < 4; ++i) t[i] = (bf16)v[i];
    *reinterpret_cast<bf16x4*>(p) = t;
}
__device__ __forceinline__ void store4(float* p, const float (&v)[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
// the same by a compile-time width W (4 or 8)
template <int W, typename T> __device__ __forceinline__ void loadv(const T* p, float (&v)[W]) { if constexpr (W == 8) load8(p, v); else load4(p, v); }
template <int W, typename T> __device__ __forceinline__ void storev(T* p, const float (&v)[W]) { if constexpr (W == 8) store8(p, v); else store4(p, v); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
// block reductions over blockDim.x (multiple of 64, <= 1024); `sh` needs 16 floats; all threads get the result
__device__ __forceinline__ float block_sum(float v, float* sh) {
    v = wave_sum(v);
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    __syncthreads();
    float r = 0.f;
    for (int i = 0; i < nw; ++i) r += sh[i];
    return r;
}
__device__ __forceinline__ float block_max(float v, float* sh) {
    v = wave_max(v);
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    __syncthreads();
    float r = -INFINITY;
    for (int i = 0; i < nw; ++i) r = fmaxf(r, sh[i]);
    return r;
}

// Activations on the fast hardware ops (v_exp_f32 = 2^x, v_rcp_f32).  exp2 of a large positive argument gives +inf and
// rcp(inf) = 0, so the saturated tails are exact without branches.
__device__ __forceinline__ float sigmoidf_(float x) {
    return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x));
}
__device__ __forceinline__ float siluf_(float x) { return x * sigmoidf_(x); }
__device__ __forceinline__ float dsiluf_(float x) { float s = sigmoidf_(x); return s * (1.f + x * (1.f - s)); }
__device__ __forceinline__ float tanhf_(float x) { return 2.f * sigmoidf_(2.f * x) - 1.f; }
// GELU, tanh approximation (reference: F.gelu(approximate='tanh'), fused_dense.py:466).  0.5(1 + tanh(y)) == sigmoid(2y),
// so  gelu(x) = x * sigmoid(2c(x + 0.044715 x^3)),  c = sqrt(2/pi):  one exp2 + one rcp per element.
__device__ __forceinline__ float geluf_(float x) {
    const float k = -2.f * 0.7978845608028654f * 1.4426950408889634f;         // -2c * log2(e)
    const float z = x * (1.f + 0.044715f * x * x);
    return x * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(k * z));
}
// gelu(x) and gelu'(x) sharing the one sigmoid (forward epilogue that saves the derivative for the backward)
__device__ __forceinline__ void gelu_both(float x, float& g, float& dg) {
    const float c2 = 2.f * 0.7978845608028654f;
    const float x2 = x * x;
    const float z = x * (1.f + 0.044715f * x2);
    const float s = __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-c2 * 1.4426950408889634f * z));
    g = x * s;
    dg = s + g * (1.f - s) * c2 * (1.f + 3.f * 0.044715f * x2);
}
__device__ __forceinline__ float dgeluf_(float x) {
    const float c2 = 2.f * 0.7978845608028654f;
    const float x2 = x * x;
    const float z = x * (1.f + 0.044715f * x2);
    const float s = __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-c2 * 1.4426950408889634f * z));
    return s + x * s * (1.f - s) * c2 * (1.f + 3.f * 0.044715f * x2);
}

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }
static inline int64_t round256(int64_t n) { return (n + 255) / 256 * 256; }    // workspace sections start on 256-byte boundaries
static inline int conv_out(long n) { return (int)((n - 1) / 2 + 1); }          // output length of a 3-tap, stride-2, pad-1 convolution
// CUs of the current device, asked for once; 256 (an MI355X) if the runtime does not say
static inline int num_cus() {
    static int cus = 0;
    if (!cus) { const int n = sconf_num_cus(); cus = n > 0 ? n : 256; }
    return cus;
}
// raises the kernels' dynamic-LDS limit the first time it is reached; `done` is a function-local static of the call site
static inline void lds_limit_once(bool& done, std::initializer_list<const void*> kernels, size_t bytes) {
    if (!done) for (const void* k : kernels) (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    done = true;
}
// read on EVERY call (tests flip them inside one process): an integer override, and SCONF_SUB_MFMA=0 (subsampler on its VALU kernels)
static inline long env_long(const char* name, long dflt) { const char* e = getenv(name); return e ? atol(e) : dflt; }
static inline bool sub_mfma_off() { const char* e = getenv("SCONF_SUB_MFMA"); return e && e[0] == '0'; }

// ---- fixed-order accumulation ----------------------------------------------------------------
// Float atomics from many workgroups onto one address add up in arrival order, which changes from run to run, and so would
// the training step.  Kernels that add ONE value per (workgroup, address) instead get a zeroed row of a slab each (they move
// their output pointers by their row * stride), and det_finish adds the rows into the real outputs in row order.  The slab is
// the caller's workspace (each entry point has a sconf_*_workspace size query), ordered on the caller's stream.
template <typename T> struct DetSegs { T* out[4]; long off[4]; long n[4]; int k; };

// slab (rows, stride): column j of segment i is added to out[i][j - off[i]].  Block = 64 columns x 16 waves; wave w sums rows
// w, w + 16, ... and wave 0 adds the 16 partial sums in order.
template <typename T>
__global__ __launch_bounds__(1024) void det_reduce_kernel(const T* __restrict__ slab, long rows, long stride, DetSegs<T> s) {
    __shared__ T red[16][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long col = (long)blockIdx.x * 64 + lane;
    T a = 0;
    if (col < stride) {
#pragma unroll 8
        for (long r = wv; r < rows; r += 16) a += slab[r * stride + col];
    }
    red[wv][lane] = a;
    __syncthreads();
    if (wv == 0 && col < stride) {
        T t = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += red[k][lane];
        for (int i = 0; i < s.k; ++i)
            if (col >= s.off[i] && col < s.off[i] + s.n[i]) s.out[i][col - s.off[i]] += t;
    }
}

// the workspace as a zeroed (rows, stride) slab of T, or nullptr when it is missing or too small
template <typename T> T* det_begin(void* ws, int64_t ws_bytes, long rows, long stride, hipStream_t st) {
    const size_t bytes = (size_t)rows * stride * sizeof(T);
    if (!ws || ws_bytes < (int64_t)bytes) return nullptr;
    if (hipMemsetAsync(ws, 0, bytes, st) != hipSuccess) return nullptr;
    return (T*)ws;
}
template <typename T> void det_finish(const T* slab, long rows, long stride, const DetSegs<T>& s, hipStream_t st) {
    hipLaunchKernelGGL(det_reduce_kernel<T>, dim3(cdiv(stride, 64)), dim3(1024), 0, st, slab, rows, stride, s);
}

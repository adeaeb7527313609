// The gfx950 primitives that hipcc has no safe spelling for, each exactly once: address-space pointers, buffer descriptors, LDS-DMA
// issued from inline asm, hand-placed waits, register ties, the 32x32 accumulator row map and the in-kernel stamp macros.
// Included by common.h after its vector typedefs.  Every asm statement names what it clobbers and the hazard it respects; a kernel
// that needs one of them calls it from here and keeps only what is specific to itself.
#pragma once

// ---- address spaces ------------------------------------------------------------------------------------------------------
typedef const __attribute__((address_space(1))) void* gptr;    // source of __builtin_amdgcn_global_load_lds
typedef __attribute__((address_space(3))) void* lptr;          // its LDS destination
typedef __attribute__((address_space(3))) bf16x4* lds_p4;      // operand of __builtin_amdgcn_ds_read_tr16_b64_v4bf16
// byte address of an LDS object (what M0, a DMA destination or an asm `ds_read` takes)
__device__ __forceinline__ unsigned lds_addr(const void* p) { return (unsigned)(size_t)(const __attribute__((address_space(3))) char*)p; }

// ---- hand-placed waits -----------------------------------------------------------------------------------------------------
// For what the compiler does not know is in flight (everything issued from asm below).  They clobber nothing; "memory" keeps the
// compiler's own accesses on their side.  vmcnt is in order and shared with the compiler's loads: N = how many younger may stay.
template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory"); }
__device__ __forceinline__ void wait_lgkm0() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
// a raw barrier behind the LDS wait only: __syncthreads() also waits for vmcnt(0), i.e. for global stores nothing depends on
__device__ __forceinline__ void wait_lgkm0_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ---- register ties ---------------------------------------------------------------------------------------------------------
// An empty asm that "rewrites" a VGPR value: no instruction, no clobber.  The compiler must have the value complete HERE (its
// loads waited for) and can neither hoist what is derived from it above the statement nor keep such results live across it.
template <typename T> __device__ __forceinline__ void tie(T& x) { asm volatile("" : "+v"(x)); }
__device__ __forceinline__ int opaque(int v) { tie(v); return v; }
// the same for a wave-uniform value in an SGPR: what is computed from the result stays scalar and is not folded into what produced x
__device__ __forceinline__ unsigned tie_s(unsigned x) { asm("" : "+s"(x)); return x; }
template <int NF> __device__ __forceinline__ void pin_frags(bf16x8 (&f)[NF]) {
#pragma unroll
    for (int i = 0; i < NF; ++i) tie(f[i]);
}

// row of register r of a 32x32 MFMA accumulator in lane half hh = lane >> 5 (the column is lane & 31)
__device__ __forceinline__ int acc_row(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }

// ---- LDS-DMA issued from inline asm ----------------------------------------------------------------------------------
// hipcc cannot tell an LDS read from the destination of an in-flight global_load_lds issued through the builtin, so it puts
// `s_waitcnt vmcnt(0)` in front of the first LDS read that follows one in program order: issued at the top of a stage, the next
// stage's tile had to LAND before the current stage could be computed (60 % of the wave-cycles of the 8-wave dK/dV attention kernel
// were parked there).  An asm statement is opaque to that bookkeeping: a kernel issues its DMA here, waits for it itself
// (`wait_vm<0>()` right before the barrier that publishes the stage) and leaves every LDS READ to the compiler.
// For that to work the loop must hold NO vector-memory operation the compiler knows of (the hardware counter is in order and
// shared: any `s_waitcnt vmcnt(N)` it emits for a load of its own - a fragment loaded before the loop whose wait it sinks to the
// first use, a spill reload, a per-stage statistics load - also waits for the DMA issued before it).
// M0 carries the wave's LDS destination base (lane l lands at M0 + l * 16, or + l * 4) and is compiler-reserved: it cannot be
// named as a clobber or an operand, so it is saved, written and restored INSIDE the one statement that reads it (`s_nop 0`: an
// SALU write of M0 needs one wait state before the LDS-DMA that uses it).  Clobbers: memory; no SCC, no VCC.
__device__ __forceinline__ void dma16_asm(const void* gsrc, unsigned lds_dst_wave_base) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst_wave_base) : "memory");
}
__device__ __forceinline__ void dma4_asm(const void* gsrc, unsigned lds_dst_wave_base) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst_wave_base) : "memory");
}

// ---- LDS-DMA through a buffer descriptor, a whole tile per asm statement -----------------------------------------------
// In-kernel stamps of the 8-wave attention forward showed the DMA ISSUE of dma16_asm on every wave's critical path: 950 cycles
// per stage for waves 0-3 and 1950 for waves 4-7 (12-25 % of the kernel) - per 16-byte piece a 64-bit address (row clamp, multiply
// by the row stride, swizzle) rebuilt on the VALU plus an M0 save / set / restore around it.  Here the per-lane part of the address
// is ONE loop-invariant 32-bit offset, the rest is scalar: `buffer_load_dwordx4 voff, srd, soff offen lds` with soff and M0
// stepped by s_add.  Rows past the tensor need no clamp: the descriptor's range check returns zeros for them.  3 scalar
// instructions + the load per piece, M0 saved and restored once per tile.
typedef __amdgpu_buffer_rsrc_t srd_t;
// raw buffer over [base, base + nbytes) (clamped to 4 GB - 1); base and size made wave-uniform
__device__ __forceinline__ srd_t make_srd(const void* base, long nbytes) {
    const unsigned long a = (unsigned long)base;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    const unsigned nb = __builtin_amdgcn_readfirstlane((unsigned)(nbytes > 0xffffffffL ? 0xffffffffL : nbytes));
    return __builtin_amdgcn_make_buffer_rsrc((void*)(((unsigned long)hi << 32) | lo), 0, nb, 0x00020000);
}
// the same over values that are ALREADY wave-uniform (kernel arguments, scalar loop state): no readfirstlane, so a descriptor that
// is rebased inside a loop costs SALU only.  A per-lane value here does not compile ("illegal VGPR to SGPR copy").
__device__ __forceinline__ srd_t make_srd_uniform(const void* base, long nbytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (unsigned)(nbytes > 0xffffffffL ? 0xffffffffL : nbytes), 0x00020000);
}
// The descriptor forms open with `s_nop 4`: the descriptor and soff may come straight out of VALU readfirstlanes, and a VALU write
// of an SGPR needs wait states before a VMEM instruction reads it that the assembler does not insert inside an asm statement.
// s_add_u32 writes SCC: the multi-piece form names "scc" as a clobber (the single-dword form has no s_add).  Both clobber memory.
// 4 bytes per lane: lds_base (uniform) + 4 * lane <- srd[soff + voff]
__device__ __forceinline__ void dma_dword(srd_t srd, unsigned voff, unsigned soff, unsigned lds_base) {
    unsigned keep;
    asm volatile("s_nop 4\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dword %3, %4, %1 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep), "+s"(soff), "+s"(lds_base) : "v"(voff), "s"(srd) : "memory");
}
// NP pieces of 16 bytes per lane: piece k reads srd base + soff + k * sstep + voff and lands at lds_wave_base + k * LSTEP + lane * 16
#define SCONF_DMA_FIRST_S "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %5\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %3, %1 offen lds\n\t"
#define SCONF_DMA_FIRST "s_nop 4\n\t" SCONF_DMA_FIRST_S
#define SCONF_DMA_NEXT  "s_add_u32 m0, m0, %6\n\ts_add_u32 %1, %1, %4\n\tbuffer_load_dwordx4 %2, %3, %1 offen lds\n\t"
#define SCONF_DMA_LAST  "s_mov_b32 m0, %0"
// one piece: dma_pieces' first step alone - the same s_nop 4, M0 save / set / s_nop 0 / restore; no s_add, so SCC stays untouched
__device__ __forceinline__ void dma_piece(srd_t srd, unsigned voff, unsigned soff, unsigned lds_wave_base) {
    unsigned keep;
    asm volatile("s_nop 4\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(srd), "s"(soff), "s"(lds_wave_base) : "memory");
}
template <int NP, int LSTEP> __device__ __forceinline__ void dma_pieces(srd_t srd, unsigned voff, unsigned soff, unsigned sstep, unsigned lds_wave_base) {
    static_assert(NP == 2 || NP == 4 || NP == 8, "tiles of 2, 4 or 8 pieces per wave");
    unsigned keep;
    if constexpr (NP == 8)
        asm volatile(SCONF_DMA_FIRST SCONF_DMA_NEXT SCONF_DMA_NEXT SCONF_DMA_NEXT SCONF_DMA_NEXT SCONF_DMA_NEXT SCONF_DMA_NEXT SCONF_DMA_NEXT SCONF_DMA_LAST
                     : "=&s"(keep), "+s"(soff) : "v"(voff), "s"(srd), "s"(sstep), "s"(lds_wave_base), "n"(LSTEP) : "memory", "scc");
    else if constexpr (NP == 4)
        asm volatile(SCONF_DMA_FIRST SCONF_DMA_NEXT SCONF_DMA_NEXT SCONF_DMA_NEXT SCONF_DMA_LAST
                     : "=&s"(keep), "+s"(soff) : "v"(voff), "s"(srd), "s"(sstep), "s"(lds_wave_base), "n"(LSTEP) : "memory", "scc");
    else
        asm volatile(SCONF_DMA_FIRST SCONF_DMA_NEXT SCONF_DMA_LAST
                     : "=&s"(keep), "+s"(soff) : "v"(voff), "s"(srd), "s"(sstep), "s"(lds_wave_base), "n"(LSTEP) : "memory", "scc");
}
// The same two forms WITHOUT the leading `s_nop 4`, for a caller whose descriptor, soff and LDS base are all written by the SALU (an
// SALU write of an SGPR needs no wait state before a VMEM read of it) on EVERY path that reaches the statement: no v_readfirstlane,
// no v_readlane reload of a spilled SGPR within 5 wait states ahead of it.  That is a property of the caller's compiled code, to be
// read off its listing (gemm256.hip: the steady K-tile loops); where it is not established, use the forms above.
__device__ __forceinline__ void dma_piece_s(srd_t srd, unsigned voff, unsigned soff, unsigned lds_wave_base) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(srd), "s"(soff), "s"(lds_wave_base) : "memory");
}
template <int NP, int LSTEP> __device__ __forceinline__ void dma_pieces_s(srd_t srd, unsigned voff, unsigned soff, unsigned sstep, unsigned lds_wave_base) {
    static_assert(NP == 2, "half-tiles of 2 pieces per wave");
    unsigned keep;
    asm volatile(SCONF_DMA_FIRST_S SCONF_DMA_NEXT SCONF_DMA_LAST
                 : "=&s"(keep), "+s"(soff) : "v"(voff), "s"(srd), "s"(sstep), "s"(lds_wave_base), "n"(LSTEP) : "memory", "scc");
}

// ---- in-kernel time stamps (cdna_hip_programming.md section 7) ---------------------------------------------------------
// DIAGNOSTIC builds only: a file turns them on by defining SCONF_STAMPS from its own -D before it includes common.h
// (attention.hip: SCONF_ATTN_STAMP, gemm256.hip: SCONF_GEMM_STAMP, ctc.hip: CTC_STAMP); in the product build the macros are empty
// and no stamp executes.  Segment sums are kept per wave and written once after the loop by the file's own STAMP_OUT, to a buffer
// nothing else reads.  The time read returns through lgkmcnt and is waited for in the statement; the sched_barriers keep the
// scheduler from moving the segment's work across the stamp.  Clobbers: memory.
#ifdef SCONF_STAMPS
#define STAMP_DECL(n) unsigned long long st_acc_[n] = {}, st_last_ = 0; { unsigned long long t_; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); st_last_ = t_; }
#define STAMP(i) do { __builtin_amdgcn_sched_barrier(0); unsigned long long t_; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); \
                      __builtin_amdgcn_sched_barrier(0); st_acc_[i] += t_ - st_last_; st_last_ = t_; } while (0)
#else
#define STAMP_DECL(n)
#define STAMP(i)
#endif

// d4g_arch.h — the one place where the two builds of the kernels part: gfx950 (hipcc) and the test-only CPU emulator
// (tests/hostsim/, -DD4G_HOSTSIM, where hipsim.h stands in for the HIP runtime).  Every device primitive whose body
// differs between them is defined here, its gfx950 body next to its emulator body; the kernel headers use only these names.
// The emulator runs a workgroup's lanes as fibers, one at a time between wave collectives (__shfl, __ballot) and workgroup
// barriers: what makes a wave wait for its own lanes on the GPU is a collective there.
#pragma once
#include <stdint.h>

#ifndef D4G_HOSTSIM
#include <hip/hip_runtime.h>
#endif

#if defined(D4G_PROFILE_OPS) && defined(D4G_HOSTSIM)
#error "D4G_PROFILE_OPS counts GPU clock cycles: the emulator build has no clock"
#endif

#define D4G_DEV __device__ __forceinline__

// The emulator's deliberate algorithm swaps.  Each wave collective costs the emulator a fiber switch per lane, so where a
// wave-wide builder has a one-lane equivalent with the same result, the emulator runs the one-lane form to keep test time
// down: the search's Huffman trees (d4g_wave_tree, d4g_rebuild.h) and Zopfli's package-merge (zf_pm, d4g_zopfli.h), the two
// places that test the switch.  The GPU always runs the wave-wide builders; -DD4G_SIM_WAVE_HEAP (tests/hostsim/build.sh
// waveheap) runs them in the emulator too.
#if defined(D4G_HOSTSIM) && !defined(D4G_SIM_WAVE_HEAP)
#define D4G_SERIAL_TREES
#endif

// Diagnostics printed by the emulator build only (the GPU build counts the same failures in c.errors)
#ifdef D4G_HOSTSIM
#define D4G_SIM_LOG(...) fprintf(stderr, __VA_ARGS__)
#else
#define D4G_SIM_LOG(...) ((void)0)
#endif

// ---------------------------------------------------------------------------------------
// Scheduling
// ---------------------------------------------------------------------------------------
// Issue priority of the optimiser's waves (s_setprio): above the default 0, so that they are not starved by an old, always-ready
// wave of another kernel on the same SIMD (the Zopfli squeeze runs for minutes); serial sections go to 3 and come back here.
#define D4G_BASE_PRIO 1
#ifdef D4G_HOSTSIM
#define D4G_SETPRIO(n) ((void)0)
// occupancy target of a kernel (caps its VGPR budget); the emulator build has no such notion
#define D4G_WAVES_PER_SIMD(n)
#else
#define D4G_SETPRIO(n) __builtin_amdgcn_s_setprio(n)   // (a macro: the builtin takes a constant)
#define D4G_WAVES_PER_SIMD(n) __attribute__((amdgpu_waves_per_eu(n, 8)))
#endif
#ifndef D4G_SPIN_SLEEP
#define D4G_SPIN_SLEEP 8
#endif

// ---------------------------------------------------------------------------------------
// Wave collectives
// ---------------------------------------------------------------------------------------
#ifdef D4G_HOSTSIM
// LDS writes of a wave's lanes are visible to its other lanes once they have all arrived here
D4G_DEV void d4g_wave_sync() { (void)__ballot(1); }   // the emulator's lanes are not in lock step: rendezvous
// The wave's vote on a condition.
D4G_DEV unsigned long long d4g_ballot(bool p) { return __ballot(p ? 1 : 0); }
// lane k's v (k wave-uniform)
D4G_DEV int d4g_readlane(int v, int k) { return __shfl(v, k); }
D4G_DEV uint32_t d4g_readlane(uint32_t v, int k) { return __shfl(v, k); }
// A wave-uniform value in a scalar register.  Every caller passes a value that is the same on all lanes, and some call with
// part of the wave (the header search's candidates run on lanes 0..55 only), where a collective would meet lanes that did
// not call: the emulator returns the value itself.
D4G_DEV int d4g_uniform(int v) { return v; }
// The lanes of a wave read LDS together.  The emulator's lanes do not: where lane 0 may rewrite what the wave has just read
// before the next collective, the wave meets here first.  Nothing on the GPU.
D4G_DEV void d4g_lockstep() { (void)__ballot(1); }
#else
// LDS writes of a wave's lanes are visible to its other lanes once they have all arrived here (the LDS executes one wave's
// operations in order; the barrier keeps the compiler from moving them across)
D4G_DEV void d4g_wave_sync() { __builtin_amdgcn_wave_barrier(); }
// The wave's vote on a condition.  (HIP's __ballot takes an int: a bool goes through 0 / 1 and a second compare.)
D4G_DEV unsigned long long d4g_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
// lane k's v (k wave-uniform): v_readlane
D4G_DEV int d4g_readlane(int v, int k) { return __builtin_amdgcn_readlane(v, k); }
D4G_DEV uint32_t d4g_readlane(uint32_t v, int k) { return (uint32_t)__builtin_amdgcn_readlane((int)v, k); }
// A wave-uniform value in a scalar register (v_readfirstlane): tells the compiler what is wave-uniform
D4G_DEV int d4g_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
D4G_DEV void d4g_lockstep() {}
#endif

// Runs fn() on every lane where p holds, one lane after another (the lanes share scratch memory).  The emulator's lanes
// already run one at a time between collectives, and a vote would meet lanes that did not call: each runs its own.
template <typename Fn>
D4G_DEV void d4g_lanes_in_turn(bool p, int lane, Fn fn) {
#ifdef D4G_HOSTSIM
    if (p) fn();
#else
    unsigned long long need = d4g_ballot(p);
    while (need) {
        const int l = __ffsll((long long)need) - 1;
        need &= need - 1;
        if (lane == l) fn();
    }
#endif
}

// 32-bit wave sum: row scans and row broadcasts on the DPP path (six v_add_u32), no LDS crossbar trips
D4G_DEV int wave_sum_i32(int v) {
#ifdef D4G_HOSTSIM
    for (int m = 32; m >= 1; m >>= 1) v = (int)((unsigned)v + (unsigned)__shfl_xor(v, m));   // wraps, as v_add_u32 (hash sums)
    return v;
#else
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);  // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);  // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);  // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);  // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);  // row_bcast:15 into rows 1 and 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);  // row_bcast:31 into rows 2 and 3
    return __builtin_amdgcn_readlane(v, 63);
#endif
}

// 32-bit unsigned wave minimum on the same DPP path (lanes a shift does not reach keep the identity ~0u)
D4G_DEV uint32_t wave_min_u32(uint32_t v) {
#ifdef D4G_HOSTSIM
    for (int m = 32; m >= 1; m >>= 1) { const uint32_t o = __shfl_xor(v, m); v = o < v ? o : v; }
    return v;
#else
    int x = (int)v;
    auto step = [&](int o) { x = (int)((uint32_t)o < (uint32_t)x ? (uint32_t)o : (uint32_t)x); };
    step(__builtin_amdgcn_update_dpp(-1, x, 0x111, 0xf, 0xf, false));  // row_shr:1
    step(__builtin_amdgcn_update_dpp(-1, x, 0x112, 0xf, 0xf, false));  // row_shr:2
    step(__builtin_amdgcn_update_dpp(-1, x, 0x114, 0xf, 0xf, false));  // row_shr:4
    step(__builtin_amdgcn_update_dpp(-1, x, 0x118, 0xf, 0xf, false));  // row_shr:8
    step(__builtin_amdgcn_update_dpp(-1, x, 0x142, 0xa, 0xf, false));  // row_bcast:15 into rows 1 and 3
    step(__builtin_amdgcn_update_dpp(-1, x, 0x143, 0xc, 0xf, false));  // row_bcast:31 into rows 2 and 3
    return (uint32_t)__builtin_amdgcn_readlane(x, 63);
#endif
}

// The value held by the lane 2^(5-D) away (the path-per-lane queue of d4g_device.h)
template <int D> D4G_DEV unsigned d4g_rp_sibling(unsigned v) {
#ifdef D4G_HOSTSIM
    return (unsigned)__shfl_xor((int)v, 32 >> D);
#else
    if (D == 0) return (unsigned)__shfl_xor((int)v, 32);
    if (D == 1) return (unsigned)__builtin_amdgcn_ds_swizzle((int)v, 0x401F);                  // swap with lane ^ 16
    if (D == 2) return (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x128, 0xf, 0xf, false);    // row_ror:8
    if (D == 3) return (unsigned)__builtin_amdgcn_ds_swizzle((int)v, 0x101F);                  // swap with lane ^ 4
    if (D == 4) return (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xf, 0xf, false);     // quad_perm [2,3,0,1]
    return (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xf, 0xf, false);                  // quad_perm [1,0,3,2]
#endif
}

// ---------------------------------------------------------------------------------------
// Bit and packed arithmetic
// ---------------------------------------------------------------------------------------
// bit p of x -> bit 2p (p < 32)
D4G_DEV unsigned long long d4g_spread_bits(unsigned x) {
#ifdef D4G_HOSTSIM
    unsigned long long v = x;
    v = (v | (v << 16)) & 0x0000ffff0000ffffull;
    v = (v | (v << 8)) & 0x00ff00ff00ff00ffull;
    v = (v | (v << 4)) & 0x0f0f0f0f0f0f0f0full;
    v = (v | (v << 2)) & 0x3333333333333333ull;
    v = (v | (v << 1)) & 0x5555555555555555ull;
    return v;
#else
    unsigned long long o;
    asm("s_bitreplicate_b64_b32 %0, %1" : "=s"(o) : "s"(x));   // every bit doubled
    return o & 0x5555555555555555ull;
#endif
}

// Byte funnel shift: the 32 bits that start sh (0..3) bytes into the little-endian pair lo, hi (v_alignbyte_b32)
D4G_DEV uint32_t d4g_alignbyte(uint32_t hi, uint32_t lo, int sh) {
#ifdef D4G_HOSTSIM
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (sh & 3)));
#else
    return __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)sh);
#endif
}

// How many of the eight 16-bit places of c0..c3 are below k (the Zopfli squeeze's change points, d4g_zopfli.h): both halves
// of a word at once with the packed 16-bit instructions (a place is below k when place - k is negative; nothing overflows:
// every value is below 2^15).
D4G_DEV int zf_count_below(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, int k) {
#ifdef D4G_HOSTSIM
    return ((int)(c0 & 0xffff) < k) + ((int)(c0 >> 16) < k) + ((int)(c1 & 0xffff) < k) + ((int)(c1 >> 16) < k) +
           ((int)(c2 & 0xffff) < k) + ((int)(c2 >> 16) < k) + ((int)(c3 & 0xffff) < k) + ((int)(c3 >> 16) < k);
#else
    typedef short zf_s2 __attribute__((ext_vector_type(2)));
    const zf_s2 kk = {(short)k, (short)k};
    zf_s2 a, b, c, d;
    __builtin_memcpy(&a, &c0, 4); __builtin_memcpy(&b, &c1, 4); __builtin_memcpy(&c, &c2, 4); __builtin_memcpy(&d, &c3, 4);
    const zf_s2 t = ((a - kk) >> 15) + ((b - kk) >> 15) + ((c - kk) >> 15) + ((d - kk) >> 15);   // -1 per place below k
    return -((int)t.x + (int)t.y);
#endif
}

// ---------------------------------------------------------------------------------------
// Memory ordering between workgroups and inside one
// ---------------------------------------------------------------------------------------
// Candidate states, masks and the flags that hand work from one workgroup to another inside a launch are written with
// agent-scope write-through stores and read with agent-scope (L1-bypassing) loads, so the hand-off needs no L2 write-back /
// L1 invalidate per task (MI355X_MICROARCH.md: "sc1 stores + drained flag", every load of the handed-off bytes an sc1 load).
// Tokens and decoded bytes are read-only and keep using plain cached loads.  The emulator runs one workgroup at a time.
#ifdef D4G_HOSTSIM
D4G_DEV int32_t d4g_ld_agent(const int32_t* p) { return *p; }
D4G_DEV uint32_t d4g_ld_agent(const uint32_t* p) { return *p; }
D4G_DEV uint64_t d4g_ld_agent(const uint64_t* p) { return *p; }
D4G_DEV void d4g_st_agent(int32_t* p, int32_t v) { *p = v; }
D4G_DEV void d4g_st_agent(uint32_t* p, uint32_t v) { *p = v; }
D4G_DEV void d4g_st_agent(uint64_t* p, uint64_t v) { *p = v; }
D4G_DEV void d4g_fence_block() {}
D4G_DEV void d4g_release_agent() {}
D4G_DEV void d4g_acquire_agent() {}
D4G_DEV void d4g_drain_stores() {}
D4G_DEV void d4g_sleep() {}
#else
D4G_DEV int32_t d4g_ld_agent(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
D4G_DEV uint32_t d4g_ld_agent(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
D4G_DEV uint64_t d4g_ld_agent(const uint64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
D4G_DEV void d4g_st_agent(int32_t* p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
D4G_DEV void d4g_st_agent(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
D4G_DEV void d4g_st_agent(uint64_t* p, uint64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
D4G_DEV void d4g_fence_block() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }
D4G_DEV void d4g_release_agent() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent"); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
D4G_DEV void d4g_acquire_agent() { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
D4G_DEV void d4g_drain_stores() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
D4G_DEV void d4g_sleep() { __builtin_amdgcn_s_sleep(D4G_SPIN_SLEEP); }
#endif

// ---------------------------------------------------------------------------------------
// Clocks (profile builds and the Zopfli squeeze's section timings; the emulator has no clock and reads 0)
// ---------------------------------------------------------------------------------------
#ifdef D4G_HOSTSIM
D4G_DEV long long d4g_wall_clock() { return 0; }
D4G_DEV long long d4g_clock_drained() { return 0; }
#else
D4G_DEV long long d4g_wall_clock() { return (long long)wall_clock64(); }
// a cycle count that is not overtaken by (and does not overtake) outstanding LDS / memory operations
D4G_DEV long long d4g_clock_drained() {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    long long t = clock64();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    return t;
}
#endif

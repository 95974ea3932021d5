// d4g_sort.h — the encoders' block sort: a stable counting sort of up to 32768 positions by a 15-bit key, by one workgroup
// of D4G_SORT_THREADS threads.  k_lz_sort (d4g_lz77.h) sorts a block's positions by zlib's hash of their three bytes,
// k_zf_sort (d4g_zopfli.h) by a key read from an array.
#pragma once
#include "d4g_device.h"

#define D4G_SORT_THREADS 512

// Positions [0, nIns) ordered by (keyOf(i), i).  All D4G_SORT_THREADS threads call.
//   tbl[32768], part[D4G_SORT_THREADS]: the caller's LDS (counts, then bucket cursors; partial sums)
//   bstartOut[key]: first slot of the key's bucket, for all 32768 keys
//   sortedOut[slot]: the position in that slot;  rankOut[i]: the slot of position i
template <typename KeyFn>
__device__ __forceinline__ void d4g_block_sort_by_key(KeyFn keyOf, int nIns, uint16_t* tbl, unsigned* part, uint16_t* bstartOut,
                                                      uint16_t* sortedOut, uint16_t* rankOut) {
    const int tid = threadIdx.x, lane = tid & 63;
    unsigned* tw = (unsigned*)tbl;
    for (int i = tid; i < 16384; i += D4G_SORT_THREADS) tw[i] = 0;
    __syncthreads();
    for (int i = tid; i < nIns; i += D4G_SORT_THREADS) {
        const unsigned h = keyOf(i);
        atomicAdd(tw + (h >> 1), 1u << ((h & 1) * 16));   // two 16-bit counters per word; a count is at most 32768
    }
    __syncthreads();
    // exclusive scan of the 32768 counters: 64 per thread
    unsigned sum = 0;
    for (int k = 0; k < 32; k++) { unsigned w = tw[tid * 32 + k]; sum += (w & 0xffffu) + (w >> 16); }
    part[tid] = sum;
    __syncthreads();
    if (tid < 64) {   // scan of 512 partial sums by one wave: 8 per lane
        unsigned loc[8], s = 0;
        for (int k = 0; k < 8; k++) { loc[k] = s; s += part[tid * 8 + k]; }
        unsigned inc = s;
        for (int dd = 1; dd < 64; dd <<= 1) { unsigned o = __shfl_up(inc, dd); if (lane >= dd) inc += o; }
        unsigned excl = inc - s;
        for (int k = 0; k < 8; k++) part[tid * 8 + k] = excl + loc[k];
    }
    __syncthreads();
    {
        unsigned run = part[tid];
        for (int k = 0; k < 32; k++) {
            unsigned w = tw[tid * 32 + k];
            unsigned a = run, b = run + (w & 0xffffu);
            run = b + (w >> 16);
            tw[tid * 32 + k] = (a & 0xffffu) | (b << 16);
            bstartOut[tid * 64 + 2 * k] = (uint16_t)a;
            bstartOut[tid * 64 + 2 * k + 1] = (uint16_t)b;
        }
    }
    __syncthreads();
    if (tid >= 64) return;
    // Placement in position order by one wave, 64 positions per step.  Lanes whose key is unique within the step take
    // their bucket's cursor directly; lanes that share a key are found by a write / read-back of lane tags in the
    // cursor table itself and ranked by ballots (a handful of groups per step on text).
    volatile uint16_t* vt = tbl;
    const unsigned long long below = lane ? (~0ULL >> (64 - lane)) : 0ULL;
    for (int i0 = 0; i0 < nIns; i0 += 64) {
        const int i = i0 + lane;
        const bool valid = i < nIns;
        unsigned h = 0;
        if (valid) h = keyOf(i);
        unsigned cur = valid ? vt[h] : 0u;
        d4g_wave_sync();
        if (valid) vt[h] = (uint16_t)(0x8000u | (unsigned)lane);
        d4g_wave_sync();
        unsigned w = valid ? vt[h] : 0u;
        d4g_wave_sync();
        if (valid && (w & 63u) != (unsigned)lane) vt[h] = (uint16_t)(0xC000u | (unsigned)lane);
        d4g_wave_sync();
        unsigned w2 = valid ? vt[h] : 0u;
        d4g_wave_sync();
        bool dup = valid && (w2 & 0x4000u);
        unsigned rank = cur;
        if (valid && !dup) vt[h] = (uint16_t)(cur + 1);
        unsigned long long rem = __ballot(dup);
        while (rem) {
            int leader = __ffsll((long long)rem) - 1;
            unsigned hh = __shfl(h, leader);
            unsigned long long m = __ballot(dup && h == hh);
            if (dup && h == hh) {
                rank = cur + (unsigned)__popcll(m & below);
                if ((m >> lane) == 1ULL) vt[h] = (uint16_t)(cur + (unsigned)__popcll(m));   // the group's last lane
            }
            rem &= ~m;
        }
        d4g_wave_sync();
        if (valid) {
            rankOut[i] = (uint16_t)rank;
            sortedOut[rank] = (uint16_t)i;
        }
    }
}

// d4g_header.h — the dynamic header's operations by one wave: rewriteHeader, removeTrailingHeaderCodes,
// replaceRLERunsWithLiteralsIfSmaller, recodeHeader (B/deflate/DeflateBlockHuffman.java) and the run list a header
// search starts from.  Both search executors call these: the level executor (d4g_ops.h) from wave 0 of its workgroup
// on the D4GState in LDS, the fused executor (d4g_fused.h) from whichever wave holds the task on its scratch.
// Every function is called by all 64 lanes of one wave and works on the memory it is handed.  The code-length tree is
// the caller's: clTree(clFreq, clLen) builds the 19-symbol tree of limit 7 (Huffman.ofRLEPacked,
// B/huffman/Huffman.java:117-134) with the executor's own builder, makes the lengths visible to the wave and returns
// the builder's error (lane 0's counts).
//
// How the pieces are cut is the level executor's register budget (k_exec_state_ops runs at its 64-register cap and spills;
// DESIGN.md §5 "Header pieces"): the symbol counts are cleared by the caller, the run's length is a callable taken inside
// the caller's own branch, the code lengths are read through the caller's reader and the pair count is handed out before
// the tree step.  Each of these, written the plain way, costs that kernel scratch memory.
#pragma once
#include "d4g_device.h"

// clFreq cleared by one wave: what d4g_wave_pack_header and d4g_wave_recode_header expect on entry (the level executor
// clears it with its workgroup, before a barrier)
D4G_DEV void d4g_wave_clear_cl_freq(uint32_t* clFreq) {
    if ((threadIdx.x & 63) < 20) clFreq[threadIdx.x & 63] = 0;
    d4g_wave_sync();
}

// Runs of the n concatenated code lengths (literal/length then distance; runs may span the boundary — A.4), found with
// ballots.  len(i) reads combined length i.  body(ch, start, v, runLen) is called once per chunk of 64 lengths by every
// lane, from converged code: the lane at a run's first length has start set and the run's value, and runLen() gives it
// the run's length.
template <typename LenFn, typename Body>
__device__ __forceinline__ void d4g_wave_runs(int n, LenFn len, Body body) {
    const int lane = threadIdx.x & 63;
    constexpr int NCH = (D4G_NLIT + D4G_NDIST) / 64;  // 5 chunks of 64 code lengths
    unsigned long long sm[NCH];
    int v[NCH];
#pragma unroll
    for (int ch = 0; ch < NCH; ch++) {
        int i = ch * 64 + lane;
        v[ch] = i < n ? len(i) : -1;
        int pv = (i > 0 && i < n) ? len(i - 1) : -2;
        sm[ch] = d4g_ballot(i < n && v[ch] != pv);
    }
#pragma unroll
    for (int ch = 0; ch < NCH; ch++) {
        int i = ch * 64 + lane;
        bool start = (sm[ch] >> lane) & 1;
        auto runLen = [&]() D4G_LAMBDA_INLINE {
            int nx = -1;
            unsigned long long m = lane == 63 ? 0ULL : (sm[ch] >> (lane + 1));
            if (m) nx = i + __ffsll((long long)m);
#pragma unroll
            for (int c2 = ch + 1; c2 < NCH; c2++)
                if (nx < 0 && sm[c2]) nx = c2 * 64 + __ffsll((long long)sm[c2]) - 1;
            if (nx < 0) nx = n;
            return nx - i;
        };
        body(ch, start, v[ch], runLen);
    }
}

// removeTrailingHeaderCodes — DeflateBlockHuffman.java:366-370 over :335-364: trailing zero lengths (in transmit order)
// are dropped one at a time while a non-zero one exists, i.e. everything up to the last non-zero length of the first
// nCl is kept.  Returns the new count.
D4G_DEV int d4g_wave_trim(const uint8_t* clLen, int nCl) {
    const int lane = threadIdx.x & 63;
    const bool nz = lane < nCl && lane < 19 && clLen[D4G_CL_ORDER[lane]] != 0;
    const unsigned long long m = d4g_ballot(nz);
    return m ? 64 - __clzll((long long)m) : nCl;
}

// rewriteHeader(flags) — DeflateBlockHuffman.java:484-577 (HuffmanTable.packCodeLengths :100-186 inside) of the n
// combined code lengths len(i).  The lane at each run's start packs that run: the pair count first, then the pairs at
// their prefix-summed position, and counts its symbols into clFreq (zero on entry).  Then the code-length code, the
// header's size and nCl trimmed from 19.
template <typename LenFn, typename ClTree>
__device__ __forceinline__ int d4g_wave_pack_header(int n, LenFn len, int flags, uint16_t* pairs, uint32_t* clFreq,
                                                    uint8_t* clLen, ClTree clTree, int& nPairsOut, int& nClOut, int& bitsOut) {
    const int lane = threadIdx.x & 63;
    int base = 0;
    d4g_wave_runs(n, len,
                  [&](int, bool start, int v, auto runLen) D4G_LAMBDA_INLINE {
                      int cnt = 0, run = 0;
                      if (start) { run = runLen(); d4g_pack_run(v, run, flags, [&](int, int, int) { cnt++; }); }
                      int incl = cnt;
                      for (int d = 1; d < 64; d <<= 1) {
                          int o = __shfl_up(incl, d);
                          if (lane >= d) incl += o;
                      }
                      int off = base + incl - cnt;
                      if (start)
                          d4g_pack_run(v, run, flags, [&](int sym, int r, int value) {
                              pairs[off++] = pair_encode(sym, r, value);
                              atomicAdd(&clFreq[sym], 1u);
                          });
                      base += __shfl(incl, 63);
                  });
    nPairsOut = base;   // (before the tree step: the level executor passes the state's own field)
    d4g_wave_sync();
    const int err = clTree(clFreq, clLen);
    int hbl = 0;
    if (lane < 19) hbl = (int)clFreq[lane] * (clLen[lane] + (lane >= 16 ? pair_extra_bits(lane) : 0));
    const int hb = 5 + 5 + 4 + 19 * 3 + wave_sum_i32(hbl);
    const int nCl = d4g_wave_trim(clLen, 19);
    nClOut = nCl; bitsOut = hb - 3 * (19 - nCl);
    return err;
}

// replaceRLERunsWithLiteralsIfSmaller — DeflateBlockHuffman.java:321-332: returns the bits saved
D4G_DEV int d4g_wave_replace_runs(uint16_t* pairs, int nPairs, const uint8_t* clLen, bool prune) {
    const int lane = threadIdx.x & 63;
    int saved = 0;
    for (int i = lane; i < nPairs; i += 64) {
        uint16_t p = pairs[i];
        if ((p & 31) >= 16 && !(p & D4G_PAIR_EXPANDED)) {
            int sym, run, value;
            pair_decode(p, sym, run, value);
            int g = pair_replace_gain(sym, run, value, prune, [&](int s) { return (int)clLen[s]; });
            if (g >= 0) { pairs[i] = p | D4G_PAIR_EXPANDED; saved += g; }
        }
    }
    saved = wave_sum_i32(saved);
    d4g_wave_sync();
    return saved;
}

// recodeHeader — DeflateBlockHuffman.java:579-629: a new code-length code for the pairs as they stand (counted into
// clFreq, zero on entry), nCl trimmed from nClIn (numCodelenLens deliberately not reset), the header's size
template <typename ClTree>
__device__ __forceinline__ int d4g_wave_recode_header(const uint16_t* pairs, int nPairs, uint32_t* clFreq, uint8_t* clLen, int nClIn, ClTree clTree,
                                                      int& nClOut, int& bitsOut) {
    const int lane = threadIdx.x & 63;
    for (int i = lane; i < nPairs; i += 64) {
        int sym, run, value;
        uint16_t p = pairs[i];
        pair_decode(p, sym, run, value);
        if (p & D4G_PAIR_EXPANDED) atomicAdd(&clFreq[value], (unsigned)run);
        else atomicAdd(&clFreq[sym], 1u);
    }
    d4g_wave_sync();
    const int err = clTree(clFreq, clLen);
    const int nCl = d4g_wave_trim(clLen, nClIn);
    int hbl = 0;
    for (int i = lane; i < nPairs; i += 64) {
        int sym, run, value;
        uint16_t p = pairs[i];
        pair_decode(p, sym, run, value);
        if (p & D4G_PAIR_EXPANDED) hbl += run * clLen[value];
        else hbl += clLen[sym] + (sym >= 16 ? pair_extra_bits(sym) : 0);
    }
    nClOut = nCl;
    bitsOut = 5 + 5 + 4 + 3 * nCl + wave_sum_i32(hbl);
    return err;
}

// What a header search shares among its 56 candidates (d4g_hdr_candidate_body, d4g_ops.h)
// the limiter's code-length tree: 16-bit queue entries (weight < 1024, node id < 64), depths in the queue's memory
typedef TreeMem<uint16_t, uint8_t, 20, 6, true> D4GHdrTree;
struct D4GHdrLds {
    alignas(16) uint8_t lens[D4G_NLIT + D4G_NDIST];
    uint8_t runV[D4G_MAXPAIRS];
    uint16_t runL[D4G_MAXPAIRS];
    int nRuns;              // runs whose packing depends on the flags (the others are summed in baseFreq)
    uint32_t baseFreq[20];  // code-length symbols contributed by the runs every candidate packs as plain literals
    alignas(16) unsigned char tree[D4GHdrTree::bytes(1)];   // the one tree deeper than 7 being rebuilt
    uint16_t fbFreq[19];
    uint8_t fbLen[19];
};

// The run list of a header search, from the n combined code lengths comb[] (visible to the wave).  HuffmanTable.pack turns
// a run of up to three equal non-zero lengths (up to two zeros) into plain literals whatever the flags: those only add to
// the symbol counts, once for all 56 candidates (H.baseFreq).  The other runs are listed for the candidates' own packing
// (H.runV, H.runL, H.nRuns; their order does not matter: candidates only count symbols and sum savings).  The caller
// makes the lists visible (a wave sync or a barrier) before the candidates read them.
D4G_DEV void d4g_wave_hs_runs(D4GHdrLds& H, const uint8_t* comb, int n) {
    const int lane = threadIdx.x & 63;
    if (lane < 20) H.baseFreq[lane] = 0;
    d4g_wave_sync();
    int ncx = 0;
    d4g_wave_runs(n, [&](int i) { return (int)comb[i]; },
                  [&](int, bool start, int v, auto runLen) D4G_LAMBDA_INLINE {
                      int run = 0;
                      if (start) run = runLen();
                      bool simple = start && (v != 0 ? run <= 3 : run <= 2);
                      bool cx = start && !simple;
                      if (simple) atomicAdd(&H.baseFreq[v], (unsigned)run);
                      unsigned long long cm = d4g_ballot(cx);
                      if (cx) {
                          int idx = ncx + __popcll(cm & ((1ULL << lane) - 1));
                          H.runV[idx] = (uint8_t)v;
                          H.runL[idx] = (uint16_t)run;
                      }
                      ncx += __popcll(cm);
                  });
    if (lane == 0) H.nRuns = ncx;
}

// d4g_rebuild.h — recodeHuffman's rebuild by one wave (B/deflate/DeflateBlockHuffman.java:670-743): the literal/length
// tree, the distance tree with its two special cases, the code-length tree of a header and the token bits of a histogram
// slot.  Both search executors call these, as they call the header pieces of d4g_header.h: the level executor (d4g_ops.h)
// from the first two waves of its workgroup on the D4GState in LDS, the fused executor (d4g_fused.h) from the waves that
// hold a rebuild task on its scratch.  Every function is called by all 64 lanes of one wave and works on the memory it is
// handed.
//
// What differs between the executors is the wave-wide tree builder and the layout of its memory: a tag names both.
#pragma once
#include "d4g_device.h"

struct D4GLevelTrees {   // the level executor: the wave-wide JDK heap in LDS
    typedef TreeMem<uint64_t, uint16_t, D4G_NLIT> Lit;
    typedef TreeMem<uint64_t, uint16_t, D4G_NDIST> Dist;
    template <int NREG, typename TM, typename FreqFn, typename OutFn>
    static D4G_DEV int build(TM& tm, int numSymbols, int limit, FreqFn freq, OutFn out) {
        return d4g_build_tree_wave<NREG>(tm, numSymbols, limit, freq, out);
    }
};
struct D4GFusedTrees {   // the fused executor: the queue in registers, handing over to the path and LDS builders by size
    typedef TreeMem<uint64_t, uint16_t, D4G_NLIT, 16, true> Lit;    // (depth scratch of the limiter path overlays the queue)
    typedef TreeMem<uint64_t, uint16_t, D4G_NDIST, 16, true> Dist;
    template <int NREG, typename TM, typename FreqFn, typename OutFn>
    static D4G_DEV int build(TM& tm, int numSymbols, int limit, FreqFn freq, OutFn out) {
        return d4g_build_tree_wave64<NREG>(tm, numSymbols, limit, freq, out);
    }
};
typedef TreeMem<uint32_t, uint8_t, 20> D4GClTree;   // the 19-symbol code-length tree, for either builder

// A wave's Huffman tree: the executor's wave-wide builder on the GPU.  The emulator runs the one-lane form unless asked
// (the switch of d4g_arch.h), and this is the search's only place that looks.  Returns the builder's error on every lane.
template <typename Builder, int NREG, typename TM, typename FreqFn, typename OutFn>
__device__ __forceinline__ int d4g_wave_tree(TM& tm, int numSymbols, int limit, FreqFn freq, OutFn out) {
#ifndef D4G_SERIAL_TREES
    return Builder::template build<NREG>(tm, numSymbols, limit, freq, out);
#else
    int err = 0;
    if ((threadIdx.x & 63) == 0) err = d4g_build_tree(tm, 1, 0, numSymbols, limit, freq, out);
    return __shfl(err, 0);
#endif
}

// code-length code of clFreq — Huffman.ofRLEPacked, B/huffman/Huffman.java:117-134: the code-length-tree step of the forms
// of d4g_header.h.  The lengths are visible to the wave on return.
template <typename Builder>
D4G_DEV int d4g_wave_cl_tree(unsigned char* treeMem, const uint32_t* clFreq, uint8_t* clLen) {
    D4GClTree tm;
    tm.carve(treeMem, 1);
    const int lane = threadIdx.x & 63;
    if (lane < 19) clLen[lane] = 0;
    d4g_wave_sync();
    const int err = d4g_wave_tree<Builder, 1>(tm, 19, 7, [&](int i) { return (unsigned)clFreq[i]; }, [&](int v, int len) { clLen[v] = (uint8_t)len; });
    d4g_wave_sync();
    return err;
}

// last used symbol + 1 of the n counts of hist
D4G_DEV int d4g_wave_last_used(const uint32_t* hist, int n) {
    int last = 0;
    for (int i = threadIdx.x & 63; i < n; i += 64)
        if (hist[i]) last = i + 1;
    return wave_max_i32(last);
}

// The literal/length tree of hist[0, 286) into litLen (zero and visible to the wave on entry).  Returns the builder's error.
template <typename Builder>
D4G_DEV int d4g_wave_lit_tree(const uint32_t* hist, uint8_t* litLen, unsigned char* treeMem, int& nLit) {
    const int last = d4g_wave_last_used(hist, 286);
    typename Builder::Lit tm;
    tm.carve(treeMem, 1);
    nLit = last;
    return d4g_wave_tree<Builder, (D4G_NLIT + 63) / 64>(tm, last, 15, [&](int i) { return hist[i]; }, [&](int v, int len) { litLen[v] = (uint8_t)len; });
}

// The distance tree of distHist[0, 30) into distLen (zero and visible to the wave on entry).  Returns the builder's error.
template <typename Builder>
D4G_DEV int d4g_wave_dist_tree(const uint32_t* distHist, uint8_t* distLen, unsigned char* treeMem, int& nDist) {
    const int lane = threadIdx.x & 63;
    const int last = d4g_wave_last_used(distHist, 30);
    const int nz = __popcll(d4g_ballot(lane < last && distHist[lane] != 0));
    if (last == 0) { nDist = 1; return 0; }   // handleZero: new HuffmanTable(1)
    nDist = last;
    if (nz <= 1) {                            // handleOne: one used distance code, length 1
        if (lane == 0) distLen[last - 1] = 1;
        return 0;
    }
    typename Builder::Dist tm;
    tm.carve(treeMem, 1);
    return d4g_wave_tree<Builder, 1>(tm, last, 15, [&](int i) { return distHist[i]; }, [&](int v, int len) { distLen[v] = (uint8_t)len; });
}

// Bits of the tokens counted in histogram slot i (h of them) — one term of recodeToHuffmanInternal's sum,
// DeflateBlockHuffman.java:759-770
D4G_DEV long long d4g_slot_token_bits(int i, unsigned h, const uint8_t* litLen, const uint8_t* distLen) {
    if (!h) return 0;
    if (i < D4G_NLIT) return (long long)h * (litLen[i] + (i >= 257 ? d4g_lsym_ebits(i) : 0));
    return (long long)h * (distLen[i - D4G_NLIT] + d4g_dsym_ebits(i - D4G_NLIT));
}

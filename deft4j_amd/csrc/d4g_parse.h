// d4g_parse.h — inflate-to-tokens on the GPU, parallel across deflate blocks.
//
// Results are those of DeflateStream.parse (B/deflate/DeflateStream.java:72-126),
// DeflateBlockHuffman.initDynamicDecoder (:892-1010) and decodeStream (:778-890): token arrays,
// decoded bytes, and one initial state per Huffman block (code lengths, header RLE pairs,
// symbol histogram, bit sizes).  The reference walks the stream serially; here
//   1. k_scan_headers     tests EVERY bit position for a plausible dynamic-block header
//                         (BTYPE, HLIT/HDIST range, complete code-length code, complete codes behind
//                         it) — brute force that a 256-CU chip does in well under a millisecond per 10 MB;
//   2. k_probe_blocks     one wave per candidate decodes the block without output and reports
//                         where it ends (speculative candidates must also have complete codes);
//                         the host links candidates into the one chain that starts at bit 0 and
//                         probes the few positions the scan cannot see (fixed / stored blocks);
//   3. k_emit_blocks      one wave per confirmed block decodes again, now writing tokens at
//                         their final offsets and the block's initial state;
//   4. k_seg_symbols / k_seg_compose / k_seg_substitute   decoded bytes block by block: 16-bit symbols
//                         with markers into the 32 KiB before a segment, windows resolved by a scan
//                         over segments, one substitution pass that writes U (section 4b below);
//      k_fill_src / k_jump_streams / k_resolve_streams   the same bytes by pointer jumping over the whole
//                         stream, for streams with a block too long for one workgroup (D4G_COPY).
// Decoding itself keeps the reference's semantics (LUT fast path; bit-serial canonical fallback
// identical to Huffman.readSymbol, B/huffman/Huffman.java:170-197; reads past EOF fail).
#pragma once
#include <type_traits>

#include "d4g_device.h"

struct D4GStreamDesc {
    const uint8_t* data;   // compressed bytes (device, 16-byte aligned, readable 16 KiB past len)
    long long len;
    long long uBase;       // start of this stream's region in U / src
    long long uLen;
    // preset dictionary (inflateSetDictionary): the last dictLen <= 32768 bytes of it, in device memory, shared by every stream
    // of the batch that names it.  A distance d at decoded position p is valid iff d <= p + dictLen, and position q < 0 reads
    // dict[dictLen + q].  nullptr / 0: no dictionary.
    const uint8_t* dict;
    long long dictLen;
};

struct D4GProbeIn {
    int32_t stream;
    int32_t strict;        // 1: speculative candidate (dynamic only, complete codes required)
    long long bitPos;
};
struct D4GProbeOut {
    int32_t status;        // 0 ok, -1 not a (valid) block
    int32_t type;
    int32_t bfinal;
    int32_t eofHit;        // stored block ran past the end of input (bytes read as 0xff)
    long long endBit;      // first bit after the block
    long long nTok, uLen, sizeBits;
    long long needHist;    // max over back-references of (distance - bytes produced so far in the block)
    int32_t nRef;          // back-reference tokens in the block
    int32_t firstBatch;    // first record of the block's verified chunk starts (D4GChunkBatch chain), < 0: none
    int32_t hdrBits;       // dynamic block: bits of its code-length header (after the 3 block bits), else 0
    int32_t pad;
};
// What the probe learned about a batch of 64 chunks, kept for the emit pass: per lane the verified start (bits from
// the block's first token) and its counts, so the emit decodes every chunk exactly once.
struct D4GChunkBatch {
    int32_t next;          // following batch of the same block, -1: last
    int32_t pad[3];
    uint4 rec[64];         // .x start, .y tokens | records << 10 | stop flag << 20, .z decoded bytes, .w token bits
};
struct D4GChunkPool { D4GChunkBatch* batches; unsigned* next; unsigned cap; };
struct D4GEmitIn {
    int32_t stream;
    int32_t type;
    long long bitPos;
    long long tokStart;    // absolute index into tok
    long long uStart;      // stream-relative offset of the block's decoded bytes
    long long uLen;
    long long stateIdx;    // absolute index into the state pool (slot 0 of the block), -1 for stored
    long long sizeBits;    // from the probe
    long long refStart;    // absolute index of the block's first back-reference record
    int32_t firstBatch;    // the probe's chunk records for this block (< 0: decode speculatively again)
    int32_t pad;
};
#define D4G_LUT_BITS 10
#define D4G_INCH 33024   // staged input: one batch of 512 chunks of D4G_CHUNK_BITS (32 KiB) plus the overshoot of the last token

struct D4GDecTab {          // canonical decoder of one alphabet
    uint16_t lut[1 << D4G_LUT_BITS];  // sym | len<<9, 0xffff = use the bit-serial path
    uint16_t sorted[D4G_NLIT];        // symbols ordered by (length, index)
    int first[16], count[16], offs[16];
    int useLut;
    int complete;           // Kraft sum == 1
    int nCodes;
};

#define D4G_PARSE_MAXTHREADS 512
struct D4GParseLds {
    D4GState st;
    D4GDecTab lit, dist, cl;
    alignas(16) uint8_t inbuf[D4G_INCH + 16];
    // workgroup-wide exchange of the chunk decoders: exits / stop flags, per-wave scan totals, broadcasts
    int xExit[D4G_PARSE_MAXTHREADS], xFlag[D4G_PARSE_MAXTHREADS];
    unsigned wsN[8], wsU[8], wsR[8], wsB[8];
    int wsM[8];
    int anyDirty, firstStop;
    long long bc;
};

// Bit reader owned by lane 0 (B/io/BitInputStream.java:59-82: LSB-first).
struct D4GBitReader {
    long long inBase;      // absolute byte index of inbuf[0] (multiple of 16)
    long long nbits;       // total bits of the stream
    // chunk-relative 32-bit state: the decode loop does no 64-bit position arithmetic
    int rel;               // offset in inbuf of the next byte to load into buf
    int posRel;            // bits consumed, relative to bit 8*inBase
    int limitRel;          // stream end, relative to bit 8*inBase (clamped)
    uint64_t buf;
    int cnt;
    __device__ long long pos() const { return inBase * 8 + posRel; }
    __device__ void reset_to(const uint8_t* inbuf, long long bitpos) {
        long long lim = nbits - inBase * 8;
        limitRel = lim > 0x3fffffff ? 0x3fffffff : (int)lim;
        posRel = (int)(bitpos - inBase * 8);
        rel = posRel >> 3;
        buf = 0;
        cnt = 0;
        // byte loads up to the next 4-byte boundary of the staged chunk, then aligned words
        while (rel & 3) {
            uint64_t v = (rel >= 0 && rel < D4G_INCH + 16) ? inbuf[rel] : 0;
            buf |= v << cnt;
            cnt += 8;
            rel++;
        }
        fill(inbuf);
        int sh = posRel & 7;
        buf >>= sh;
        cnt -= sh;
        fill(inbuf);
    }
    // Guarantees at least 33 valid bits (enough for one code + its extra bits).
    __device__ void fill(const uint8_t* inbuf) {
        while (cnt <= 32) {
            uint64_t v = (rel >= 0 && rel + 4 <= D4G_INCH + 16) ? *(const uint32_t*)(inbuf + rel) : 0;
            buf |= v << cnt;
            cnt += 32;
            rel += 4;
        }
    }
    __device__ int avail() const { return limitRel - posRel; }
    __device__ bool have(int n) const { return posRel + n <= limitRel; }
    __device__ void skip(int n) { buf >>= n; cnt -= n; posRel += n; }
    __device__ bool near_end() const { return rel + 1024 > D4G_INCH; }
};

#ifndef D4G_CHUNK_BITS
#define D4G_CHUNK_BITS 512   // bits per lane and pass of the wave-wide token decoder
#endif
static_assert(512 * D4G_CHUNK_BITS + 160 <= (D4G_INCH + 16) * 8, "a batch of 512 chunks must fit the staged input window");
static_assert(D4G_CHUNK_BITS + 48 < 1024, "tokens per chunk must fit the 10-bit field of a chunk record");
// 64 bits of the staged input starting at bit `posRel` (any lane, any position inside the staged chunk)
__device__ __forceinline__ uint64_t d4g_peek64(const uint8_t* inbuf, int posRel) {
    int a = (posRel >> 3) & ~3;
    int sh = posRel - a * 8;   // 0..31
    const uint32_t* w = (const uint32_t*)(inbuf + a);
    uint64_t lo = ((uint64_t)w[1] << 32) | w[0];
    uint64_t hi = w[2];
    return sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
}

// Huffman.buildCodes (B/huffman/Huffman.java:35-64) + decoder tables.  Lane 0 prepares the
// canonical structure, all lanes fill the LUT.
__device__ void d4g_build_decoder(D4GDecTab* T, const uint8_t* lens, int n) {
    const int lane = threadIdx.x, nl = blockDim.x;   // every thread of the workgroup helps
    __syncthreads();
    if (lane < 16) { T->count[lane] = 0; T->first[lane] = 0; T->offs[lane] = 0; }
    __syncthreads();
    for (int i = lane; i < n; i += nl)
        if (lens[i] > 0 && lens[i] < 16) atomicAdd(&T->count[lens[i]], 1);
    __syncthreads();
    if (lane == 0) {
        int nc = 0, next = 0, lastShift = 0, o = 0;
        long long kraft = 0;
        for (int l = 1; l <= 15; l++) {
            T->offs[l] = o;
            o += T->count[l];
            nc += T->count[l];
            if (T->count[l]) {
                next <<= (l - lastShift);
                lastShift = l;
                T->first[l] = next;
                next += T->count[l];
                kraft += (long long)T->count[l] << (15 - l);
            }
        }
        T->useLut = kraft <= (1 << 15);
        T->complete = kraft == (1 << 15);
        T->nCodes = nc;
    }
    __syncthreads();
    // symbols ordered by (length, index): symbol i sits after the lower-numbered symbols of its length
    for (int i = lane; i < n; i += nl) {
        const int l = lens[i];
        if (l > 0 && l < 16) {
            int rank = 0;
            for (int j = 0; j < i; j++) rank += lens[j] == l;
            T->sorted[T->offs[l] + rank] = (uint16_t)i;
        }
    }
    __syncthreads();
    for (int i = lane; i < (1 << D4G_LUT_BITS); i += nl) T->lut[i] = 0xffff;
    __syncthreads();
    if (T->useLut) {
        for (int l = 1; l <= D4G_LUT_BITS; l++) {
            int cnt = T->count[l];
            for (int k = lane; k < cnt; k += nl) {
                int code = T->first[l] + k;
                int sym = T->sorted[T->offs[l] + k];
                unsigned r = 0;
                for (int bI = 0; bI < l; bI++) r |= ((code >> bI) & 1u) << (l - 1 - bI);
                for (unsigned e = r; e < (1u << D4G_LUT_BITS); e += (1u << l)) T->lut[e] = (uint16_t)(sym | (l << 9));
            }
        }
    }
    __syncthreads();
}

// Decode one symbol from `bits` (lane 0), `avail` = bits left in the stream.
// Returns sym | len << 16, or -1 on failure.  (Packed return instead of an out-pointer: a generic
// pointer to a private variable next to LDS table reads trips a gfx950 backend assertion in ROCm 7.2.)
__device__ __forceinline__ int d4g_decode_sym_packed(const D4GDecTab* T, uint64_t bits, int avail) {
    unsigned e = T->lut[bits & ((1u << D4G_LUT_BITS) - 1)];
    if (e != 0xffff) {
        int l = e >> 9;
        if (l > avail) return -1;
        return (int)(e & 511) | (l << 16);
    }
    int code = 0;
    for (int l = 1; l <= 15; l++) {  // Huffman.readSymbol, bit-serial
        if (l > avail) return -1;
        code = (code << 1) | (int)((bits >> (l - 1)) & 1);
        if (T->count[l] && code >= T->first[l] && code < T->first[l] + T->count[l])
            return (int)T->sorted[T->offs[l] + code - T->first[l]] | (l << 16);
    }
    return -1;
}
#define D4G_DECODE(T, bits, avail, symVar, lenVar)            \
    do {                                                      \
        int _r = d4g_decode_sym_packed(T, bits, avail);       \
        symVar = _r < 0 ? -1 : (_r & 0xffff);                 \
        lenVar = _r < 0 ? 0 : (_r >> 16);                     \
    } while (0)

// ---------------------------------------------------------------------------------------
// 1. Header scan: which bit positions are worth a probe.  One workgroup per tile of a stream, one launch, three phases
// over the tile's bytes staged in LDS, each phase fed by a compacted list of the one before it:
//   A  every bit position: the 13-bit prolog (BTYPE = dynamic, HLIT <= 29, HDIST <= 29)              -> list A
//   B  list A, one lane per entry: the code-length code is complete (Kraft sum) and has two codes   -> list B,
//      the scan's candidates (stats.scan_candidates)
//   C  list B, one lane per entry, packed into one wave: the walk over the coded code lengths
//      (d4g_header_survives)                                                                        -> the global list
// A plausible prolog and a complete code-length code at a random bit position are common (22 % and 0.09 % of all
// positions in zlib output); the probe would spend a whole workgroup and ~300 serial symbol decodes on each, the walk
// leaves little more than the stream's true blocks.  A full list is drained through the next phase and scanning goes on:
// no list size drops a position or lets it past a test.
// ---------------------------------------------------------------------------------------
#ifndef D4G_SCAN_TILE
#define D4G_SCAN_TILE 4096   // bytes of a stream per workgroup
#endif
// A header begun in the tile's last bit ends at most 17 + 19 x 3 + 316 x 14 = 4498 bits (563 bytes) later, and the walk's
// window reads 12 bytes from its position; rounded to the 16-byte staging loads.  The input buffer is readable this far
// past any stream's end: Batch::create pads the input buffer with D4G_INCH + 64 bytes for the block decoders' staging.
#define D4G_SCAN_HALO 576
#ifndef D4G_SCAN_LIST_A
#define D4G_SCAN_LIST_A 2048   // prolog passers collected before phase B runs
#endif
#ifndef D4G_SCAN_LIST_B
#define D4G_SCAN_LIST_B 1024   // candidates collected before phase C runs
#endif
// The prolog wants bit 1 clear and bit 2 set, so no two neighbouring positions pass: 256 bytes hold at most 1024 passers.
#define D4G_SCAN_ROUNDS_A (D4G_SCAN_LIST_A / 1024)
static_assert(D4G_SCAN_LIST_A >= 1024 && D4G_SCAN_LIST_A % 1024 == 0, "list A holds whole rounds of 256 bytes");
static_assert(D4G_SCAN_LIST_B >= 256, "list B holds at least what one pass of the workgroup over list A can add");
static_assert(D4G_SCAN_TILE % 256 == 0 && D4G_SCAN_TILE * 8 <= 65536, "tile-relative bit offsets are 16-bit list entries");
static_assert(D4G_SCAN_TILE + D4G_SCAN_HALO <= D4G_INCH, "a stream's last tile and its halo are staged from inside the input buffer's padding");
static_assert((D4G_SCAN_TILE * 8 + 4498 + 31) / 32 + 3 <= (D4G_SCAN_TILE + D4G_SCAN_HALO) / 4, "the halo holds the longest header and its window");

// Bits of a staged tile for d4g_header_survives: positions count from the first bit of `words`.
struct D4GStagedBits {
    const uint32_t* words;
    __device__ __forceinline__ uint64_t peek(int p) const {   // 64 bits at bit p
        const int w = p >> 5, sh = p & 31;
        const uint64_t lo = words[w] | ((uint64_t)words[w + 1] << 32);
        const uint64_t hi = words[w + 2];
        return sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
    }
    __device__ __forceinline__ uint32_t peek32(int p) const {   // 32 bits at bit p
        return d4g_alignbit(words[(p >> 5) + 1], words[p >> 5], p & 31);
    }
};

// Phase C's predicate on one candidate (prolog at bit `pos` of `src`, the stream ends at bit `nbits`; both count from
// src's first bit).  The lane walks the coded code lengths with a private 128-entry decode table (T, CLN: the lane's
// slices of LDS, elements `stride` bytes apart), keeping only the Kraft sums: a candidate survives when its literal/length
// code is complete with an end-of-block code and its distance code is complete or has at most one code — the conditions
// the strict probe applies (d4g_parse_block), so nothing the probe would accept is dropped.  The candidate's code-length code must be
// complete (phase B's test): its table build then writes all 128 entries of T, which therefore needs no clearing between
// candidates and holds no entry without a code.
template <class Src>
__device__ __forceinline__ bool d4g_header_survives(const Src& src, int pos, const int nbits, uint8_t* T, uint8_t* CLN, const int stride) {
    uint64_t b = src.peek(pos);
    const int nLit = (int)((b >> 3) & 31) + 257;
    const int nDist = (int)((b >> 8) & 31) + 1;
    const int nCl = (int)((b >> 13) & 15) + 4;
    if (!(((b >> 1) & 3) == 2 && nLit <= 286 && nDist <= 30 && pos + 17 + 3 * nCl <= nbits)) return false;
    pos += 17;
    // 19 x 3 bits = 57 bits: one window.  Counts and next codes per length live in 8-bit fields of a word
    // (no dynamically indexed register arrays); the lengths themselves in the lane's LDS slice.
    const uint64_t c = src.peek(pos);
    uint64_t cnt64 = 0;
    for (int k = 0; k < 19; k++) CLN[k * stride] = 0;
    for (int i = 0; i < nCl; i++) {
        const int l = (int)((c >> (3 * i)) & 7);
        CLN[D4G_CL_ORDER[i] * stride] = (uint8_t)l;
        if (l) cnt64 += 1ULL << (8 * l);
    }
    pos += 3 * nCl;
    // canonical codes (Huffman.buildCodes), LUT over 7 bits (LSB-first windows: codes are bit-reversed)
    uint64_t next64 = 0;
    int code = 0;
    for (int l = 1; l <= 7; l++) {
        code = (code + (l > 1 ? (int)((cnt64 >> (8 * (l - 1))) & 255) : 0)) << 1;
        next64 |= (uint64_t)(code & 255) << (8 * l);
    }
#pragma unroll 1
    for (int k = 0; k < 19; k++) {
        const int l = CLN[k * stride];
        if (l) {
            const int cd = (int)((next64 >> (8 * l)) & 255);
            next64 += 1ULL << (8 * l);
            unsigned r = 0;
            for (int bI = 0; bI < l; bI++) r |= ((cd >> bI) & 1u) << (l - 1 - bI);
            for (unsigned e = r; e < 128; e += (1u << l)) T[e * stride] = (uint8_t)(k | (l << 5));
        }
    }
    const int combined = nLit + nDist;
    // The walk itself, in 32-bit arithmetic (a complete code of up to 286 lengths sums to 2^15; 316 x 2^14 fits easily).
    unsigned kraftLit = 0, kraftDist = 0;
    int i = 0, prev = 0, nDistCodes = 0, eob = 0;
    uint32_t win = 0;
    int have = 0;   // bits of win still ahead of pos: a step takes at most 7 + 7, so the window is fetched again below 14
    while (i < combined) {
        if (pos + 14 > nbits + 64) return false;
        if (have < 14) { win = src.peek32(pos); have = 32; }
        const unsigned e = T[(win & 127) * stride];
        const int sym = (int)(e & 31), l = (int)(e >> 5);
        win >>= l;
        // 16: repeat the previous length 3..6 times (2 extra bits); 17 / 18: 3..10 / 11..138 zeros (3 / 7 extra bits)
        const int k = sym - 16;
        const bool rep = k >= 0;
        const int extra = rep ? (0x070302 >> (8 * k)) & 0xff : 0;
        const int run = rep ? ((0x0b0303 >> (8 * k)) & 0xff) + (int)(win & ((1u << extra) - 1)) : 1;
        const int value = rep ? (k == 0 ? prev : 0) : sym;
        if (k == 0 && i < 1) return false;
        win >>= extra;
        pos += l + extra;
        have -= l + extra;
        if (pos > nbits || i + run > combined) return false;
        if (value) {
            // the run may span the literal/distance boundary
            const int inLit = i < nLit ? (i + run <= nLit ? run : nLit - i) : 0;
            kraftLit += (unsigned)inLit << (15 - value);
            kraftDist += (unsigned)(run - inLit) << (15 - value);
            nDistCodes += run - inLit;
            if (i <= 256 && i + run > 256) eob = 1;
        }
        prev = value;
        i += run;
    }
    return kraftLit == (1 << 15) && eob && (kraftDist == (1 << 15) || nDistCodes <= 1);
}

// tileStart: per stream the index of its first tile, nStreams + 1 entries (a stream's tiles are consecutive workgroups).
// counters[0] counts the survivors (also those past capKept: the host sizes the list again), counters[1] list B's entries.
__global__ void __launch_bounds__(256, 8) k_scan_headers(const D4GStreamDesc* streams, const uint32_t* tileStart, unsigned nStreams, D4GProbeIn* kept,
                                                      unsigned* counters, unsigned capKept) {
    alignas(16) __shared__ uint8_t buf[D4G_SCAN_TILE + D4G_SCAN_HALO];
    __shared__ uint8_t lut[128 * 64];     // phase C, per lane: 7-bit window -> sym | len << 5; lane-interleaved (entry e of lane j at e * 64 + j)
    __shared__ uint8_t clens[20 * 64];    // phase C, per lane: the code-length code's lengths, interleaved the same way
    __shared__ uint16_t listA[D4G_SCAN_LIST_A], listB[D4G_SCAN_LIST_B];   // bit offsets inside the tile
    __shared__ unsigned cntA, cntB;       // entries ever added; the lists hold those from baseA / baseB on
    unsigned sLo = 0, sHi = nStreams;     // the last stream whose first tile is not after this one
    while (sHi - sLo > 1) {
        const unsigned mid = (sLo + sHi) >> 1;
        if (tileStart[mid] <= blockIdx.x) sLo = mid; else sHi = mid;
    }
    const int stream = (int)sLo;
    const long long byteStart = (long long)(blockIdx.x - tileStart[sLo]) * D4G_SCAN_TILE;
    const D4GStreamDesc sd = streams[stream];
    if (threadIdx.x == 0) { cntA = 0; cntB = 0; }
    for (int i = threadIdx.x * 16; i < D4G_SCAN_TILE + D4G_SCAN_HALO; i += blockDim.x * 16)
        *(uint4*)(buf + i) = *(const uint4*)(sd.data + byteStart + i);  // the input buffer is padded past len
    __syncthreads();
    const long long tileBit0 = byteStart * 8;
    const long long restBits = sd.len * 8 - tileBit0;   // the stream's end, from the tile's first bit (> 0: the tile begins inside it)
    const int nbits = restBits > 0x3fffffff ? 0x3fffffff : (int)restBits;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ULL << lane) - 1;
    // (the waves that run phase C alone take turns from tile to tile, so that those of a compute unit's resident workgroups
    // do not all sit on one SIMD)
    const int waveC = (int)(blockIdx.x & 3);
    const long long restBytes = sd.len - byteStart;
    const int nRounds = restBytes >= D4G_SCAN_TILE ? D4G_SCAN_TILE / 256 : (int)((restBytes + 255) / 256);   // 256-byte rounds that hold any of the stream
    unsigned baseA = 0, baseB = 0;

    // Phases A, B and C take turns: after every D4G_SCAN_ROUNDS_A rounds of phase A, phase B empties list A; phase C empties
    // list B when a pass of phase B might overfill it, and behind the last round.  (One place in the code for each phase:
    // inlined at two, the walk and its table build made the kernel eight times as long.)
    for (int r0 = 0;; r0 += D4G_SCAN_ROUNDS_A) {
        const bool last = r0 >= nRounds;   // the turn behind the last round only empties list B
        // Phase A: a thread takes the 8 positions of a byte, 256 bytes a round; a wave adds its round to the list with one atomic
        for (int r = r0; !last && r < r0 + D4G_SCAN_ROUNDS_A && r < nRounds; r++) {
            const int by = r * 256 + (int)threadIdx.x;
            const uint32_t* bw = (const uint32_t*)buf + (by >> 2);
            const uint32_t x = d4g_alignbit(bw[1], bw[0], (by & 3) * 8);   // 32 bits from the byte on: 7 + 13 are needed
            unsigned long long m[8];   // per position of the byte: the wave's lanes that pass (uniform: scalar registers)
            unsigned total = 0;
#pragma unroll
            for (int s = 0; s < 8; s++) {
                const uint32_t v = x >> s;
                m[s] = __ballot(((v >> 1) & 3) == 2 && ((v >> 3) & 31) <= 29 && ((v >> 8) & 31) <= 29);
                total += (unsigned)__popcll(m[s]);
            }
            unsigned base = 0;
            if (lane == 0 && total) base = atomicAdd(&cntA, total);
            base = __shfl(base, 0) - baseA;
#pragma unroll
            for (int s = 0; s < 8; s++) {
                if ((m[s] >> lane) & 1) listA[base + (unsigned)__popcll(m[s] & below)] = (uint16_t)(by * 8 + s);
                base += (unsigned)__popcll(m[s]);
            }
        }
        __syncthreads();
        const unsigned nA = cntA - baseA;
        unsigned heldB = cntB - baseB;
        __syncthreads();   // (both counts read before anyone adds to them again)
        const bool tight = heldB + nA > D4G_SCAN_LIST_B;   // list B may fill up on the way: look before every pass
        unsigned at = 0;
        for (;;) {
            // Phase B over list A, 256 entries a pass
            bool drain = last;
            for (; at < nA; at += 256) {
                if (tight) {
                    __syncthreads();
                    heldB = cntB - baseB;
                    __syncthreads();
                    if (heldB + 256 > D4G_SCAN_LIST_B) { drain = true; break; }
                }
                const unsigned idx = at + threadIdx.x;
                bool ok = idx < nA;
                unsigned q = 0;
                if (ok) {
                    q = listA[idx];
                    // 96 bits starting at the position's byte: four aligned words of the tile, shifted into place
                    const int by = (int)(q >> 3), s = (int)(q & 7);
                    const uint32_t* bw = (const uint32_t*)buf + (by >> 2);
                    const int bsh = (by & 3) * 8;
                    const uint32_t w0 = bw[0], w1 = bw[1], w2 = bw[2], w3 = bw[3];
                    const uint64_t lo = (uint64_t)d4g_alignbit(w1, w0, bsh) | ((uint64_t)d4g_alignbit(w2, w1, bsh) << 32);
                    const uint32_t hi = d4g_alignbit(w3, w2, bsh);
                    const uint64_t v = s ? ((lo >> s) | ((uint64_t)hi << (64 - s))) : lo;   // window bits 0..63
                    const uint64_t w = (v >> 32) | ((uint64_t)(hi >> s) << 32);             // window bits 32..95
                    const int ncl = (int)((v >> 13) & 15) + 4;
                    ok = (int)q + 17 + 3 * ncl <= nbits;
                    if (ok) {
                        // the code-length code must be complete: sum 2^(7-l) == 128, at least two codes.  Branch-free over the
                        // 3-bit fields: bit planes of the (masked) 57-bit field, one popcount per length value
                        uint64_t f = (v >> 17) | ((w >> 32) << 47);           // window bits 17..80
                        f &= (1ULL << (3 * ncl)) - 1;
                        const uint64_t M = 0x1249249249249249ULL;              // bit 0 of every 3-bit field
                        const uint64_t p0 = f & M, p1 = (f >> 1) & M, p2 = (f >> 2) & M;
                        const uint64_t n0 = ~p0, n1 = ~p1, n2 = ~p2;
                        const int kraft = 64 * __popcll(p0 & n1 & n2) + 32 * __popcll(n0 & p1 & n2) + 16 * __popcll(p0 & p1 & n2) +
                                          8 * __popcll(n0 & n1 & p2) + 4 * __popcll(p0 & n1 & p2) + 2 * __popcll(n0 & p1 & p2) + __popcll(p0 & p1 & p2);
                        const int used = __popcll(p0 | p1 | p2);
                        ok = kraft == 128 && used >= 2;
                    }
                }
                // (a ballot and one LDS atomic per wave: an atomic per lane on one counter was most of an earlier scan's time)
                const unsigned long long m = __ballot(ok);
                if (m) {
                    unsigned base = 0;
                    if (lane == 0) base = atomicAdd(&cntB, (unsigned)__popcll(m));
                    base = __shfl(base, 0) - baseB;
                    if (ok) listB[base + (unsigned)__popcll(m & below)] = (uint16_t)q;
                }
            }
            if (!drain) break;
            // Phase C over list B (every thread comes here behind a barrier that follows list B's last entry).  Survivors are
            // rare: they go straight to the global list, one atomic per 64 candidates that hold any.
            const unsigned nB = cntB - baseB;
            if (wave == waveC) {
                const D4GStagedBits src = {(const uint32_t*)buf};
                for (unsigned atB = 0; atB < nB; atB += 64) {
                    bool ok = atB + lane < nB;
                    const int q = ok ? listB[atB + lane] : 0;
                    if (ok) ok = d4g_header_survives(src, q, nbits, lut + lane, clens + lane, 64);
                    const unsigned long long m = __ballot(ok);
                    if (m) {
                        unsigned g = 0;
                        if (lane == 0) g = atomicAdd(&counters[0], (unsigned)__popcll(m));
                        g = __shfl(g, 0) + (unsigned)__popcll(m & below);
                        if (ok && g < capKept) { D4GProbeIn c; c.stream = stream; c.strict = 1; c.bitPos = tileBit0 + q; kept[g] = c; }
                    }
                }
            }
            baseB += nB;
            __syncthreads();
            if (at >= nA) break;
        }
        baseA += nA;
        __syncthreads();   // list A is free again, list B complete so far
        if (last) break;
    }
    if (threadIdx.x == 0 && cntB) atomicAdd(&counters[1], cntB);
}

// ---------------------------------------------------------------------------------------
// 2./3. Block parser: one wave per block.  EMIT = false probes (counts, end position),
// EMIT = true writes tokens and the block's initial state.
// ---------------------------------------------------------------------------------------
struct D4GParseOut {
    uint2* tok;
    uint8_t* U;
    D4GState* states;
    uint4* refs;        // back-reference records (d4g_types.h), in token order; .z/.w are filled in after the bytes are resolved
    uint32_t* tokRef;   // per token: index of its back-reference record (written for back-references only)
};

// Diagnosis of a block that does not parse (k_diagnose_blocks): the reasons are the D4G_PARSE_* codes of include/deft4g.h.
enum { D4G_DIAG_OK = 0, D4G_DIAG_EOF, D4G_DIAG_BLOCK_TYPE, D4G_DIAG_STORED_LENGTHS, D4G_DIAG_CODE_LENGTHS, D4G_DIAG_LITLEN_SYMBOL,
       D4G_DIAG_DIST_SYMBOL, D4G_DIAG_DISTANCE_TOO_FAR };
struct D4GDiagIn { int32_t stream; int32_t pad; long long bitPos; long long hist; };   // the failing block; bytes decoded before it
struct D4GDiagOut { int32_t reason; int32_t pad; long long bitPos, decoded, value; };
struct D4GDiagRec { int reason, firstFar; long long bitPos, decoded, value; };          // the workgroup's record (LDS)

// Why did no code match?  0: one did (sym | len << 16 in `packed`, as d4g_decode_sym_packed returns it); D4G_DIAG_EOF: the input
// ended inside the code (fewer bits remain than the longest code has, and no code of the bits that remain matches); else -1:
// the bits are no code of this table.
__device__ inline int d4g_diag_code(const D4GDecTab* T, uint64_t bits, int avail, int& packed) {
    // (the bit-serial walk of d4g_decode_sym_packed, kept apart from it: that function is on the parse's hot path and stays
    // exactly as measured; its LUT path finds the same symbol, since a prefix code has one match)
    int code = 0, maxLen = 0;
    for (int l = 1; l <= 15; l++) if (T->count[l]) maxLen = l;
    for (int l = 1; l <= 15 && l <= avail; l++) {
        code = (code << 1) | (int)((bits >> (l - 1)) & 1);
        if (T->count[l] && code >= T->first[l] && code < T->first[l] + T->count[l]) {
            packed = (int)T->sorted[T->offs[l] + code - T->first[l]] | (l << 16);
            return 0;
        }
    }
    packed = -1;
    return avail < maxLen ? D4G_DIAG_EOF : -1;
}
// The token that starts at `bits` and does not decode: reason, offset of the failing element from the token's first bit
// (EOF: the code or extra-bit field that could not be read in full; a symbol error: the token itself), offending value.
__device__ inline void d4g_diag_token(const D4GDecTab* lit, const D4GDecTab* dist, uint64_t bits, int avail, int& reason, int& off,
                                      int& value) {
    int pk;
    off = 0; value = -1;
    int c = d4g_diag_code(lit, bits, avail, pk);
    if (c) { reason = c == D4G_DIAG_EOF ? D4G_DIAG_EOF : D4G_DIAG_LITLEN_SYMBOL; return; }
    const int sym = pk & 0xffff;
    int used = pk >> 16;
    if (sym > 285) { reason = D4G_DIAG_LITLEN_SYMBOL; value = sym; return; }
    if (sym <= 256) { reason = D4G_DIAG_OK; return; }   // (a token that decodes: not what the parser stopped at)
    const int eb = d4g_lsym_ebits(sym);
    if (used + eb > avail) { reason = D4G_DIAG_EOF; off = used; return; }
    used += eb;
    c = d4g_diag_code(dist, bits >> used, avail - used, pk);
    if (c == D4G_DIAG_EOF) { reason = D4G_DIAG_EOF; off = used; return; }
    if (c) { reason = D4G_DIAG_DIST_SYMBOL; return; }
    const int ds = pk & 0xffff;
    if (ds > 29) { reason = D4G_DIAG_DIST_SYMBOL; value = ds; return; }
    used += pk >> 16;
    if (used + d4g_dsym_ebits(ds) > avail) { reason = D4G_DIAG_EOF; off = used; return; }
    reason = D4G_DIAG_OK;
}

// DIAG (k_diagnose_blocks): the block is known not to parse; the same decode, but every way out records why in `dg`, and the
// token loop goes on past an invalid code to find the first failure in token order (`hist` = bytes decoded before the block).
// PART (k_recover_count / k_recover_emit): the block is known not to parse after `budget` decoded bytes (the diagnosis says
// so); the same decode, but only the tokens that fit the budget are counted (EMIT: written, at most capTok tokens and
// capRef records).  No state, histogram or chunk record is kept for such a block.
template <bool EMIT, bool DIAG = false, bool PART = false>
__device__ __forceinline__ void d4g_parse_block(const D4GStreamDesc& sd, long long bitPos, int strict, D4GProbeOut& po,
                                const D4GEmitIn* em, const D4GParseOut& out, const D4GChunkPool& pool, D4GDiagRec* dg = nullptr,
                                long long hist = 0, long long budget = 0, long long capTok = 0, long long capRef = 0) {
    static_assert(!(EMIT && DIAG), "a diagnosis writes no tokens");
    static_assert(!(PART && DIAG), "the diagnosis comes first: a partial decode follows its answer");
    __shared__ D4GParseLds L;
    const int tid = threadIdx.x, NL = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = NL >> 6;
    D4GBitReader br;   // thread 0's
    br.inBase = 0;
    br.nbits = sd.len * 8;
    br.rel = 0; br.posRel = 0; br.limitRel = 0; br.buf = 0; br.cnt = 0;
    D4GState* S = &L.st;
    // DIAG: one thread records the failure (element position, decoded bytes before it, offending value)
    [[maybe_unused]] auto diag = [&](int reason, long long bit, long long decoded, long long value) D4G_LAMBDA_INLINE {
        if constexpr (DIAG) { dg->reason = reason; dg->bitPos = bit; dg->decoded = decoded; dg->value = value; }
    };
    // workgroup-wide exchange of small values (all threads call; the value of thread 0 / a reduction comes back to all)
    auto bcast = [&](long long v) D4G_LAMBDA_INLINE {
        __syncthreads();
        if (tid == 0) L.bc = v;
        __syncthreads();
        return L.bc;
    };
    auto stage = [&](long long bitpos) {
        long long base = (bitpos >> 3) & ~15LL;
        if (base > sd.len) base = sd.len & ~15LL;
        __syncthreads();
        for (int i = tid * 16; i < D4G_INCH + 16; i += NL * 16) *(uint4*)(L.inbuf + i) = *(const uint4*)(sd.data + base + i);
        __syncthreads();
        br.inBase = base;
        if (tid == 0) br.reset_to(L.inbuf, bitpos);
    };
    po.nRef = 0; po.firstBatch = -1; po.hdrBits = 0; po.pad = 0;
    po.status = -1; po.type = 0; po.bfinal = 0; po.eofHit = 0; po.endBit = 0; po.nTok = 0; po.uLen = 0; po.sizeBits = 0; po.needHist = 0;
    stage(bitPos);
    long long pk = 0;
    if (tid == 0) {
        if (!br.have(3)) {
            pk = -1;
            if constexpr (DIAG) diag(D4G_DIAG_EOF, bitPos, hist, -1);
        } else { pk = (long long)(br.buf & 7); br.skip(3); }
    }
    pk = bcast(pk);
    if (pk < 0) return;
    po.bfinal = (int)(pk & 1);
    int btype = (int)(pk >> 1);
    po.type = btype;
    if (btype == 3) {
        if constexpr (DIAG) { if (tid == 0) diag(D4G_DIAG_BLOCK_TYPE, bitPos, hist, 3); }
        return;
    }
    if (strict && btype != 2) return;
    if constexpr (PART) {
        if (btype == 0) return;   // (a stored block fails in its header only: nothing of it is recovered)
    }
    if (btype == 0) {
        // DeflateBlockUncompressed.parse — B/deflate/DeflateBlockUncompressed.java:23-36
        // BitInputStream.readBits returns -1 once EOF is hit (B/io/BitInputStream.java:59-82) and `-1 & 0xffff` is
        // 0xffff: a cut-off LEN reads as 0xffff, which no NLEN (also 0xffff by then) matches; a cut-off NLEN reads as
        // 0xffff, which matches LEN == 0.  The reader is then at EOF, so a following block fails its 3-bit read.
        long long r = 0, p = 0;
        if (tid == 0) {
            p = (br.pos() + 7) & ~7LL;
            if (p + 16 > br.nbits) {
                r = -1;
                if constexpr (DIAG) diag(D4G_DIAG_EOF, p, hist, -1);
            } else {
                br.reset_to(L.inbuf, p);
                int len = (int)(br.buf & 0xffff), nlen = p + 32 > br.nbits ? 0xffff : (int)((br.buf >> 16) & 0xffff);
                r = nlen != ((~len) & 0xffff) ? -1 : len;
                if constexpr (DIAG) {   // a NLEN the input no longer holds is the end of input, not a mismatch
                    if (r < 0 && p + 32 > br.nbits) diag(D4G_DIAG_EOF, p + 16, hist, -1);
                    else if (r < 0) diag(D4G_DIAG_STORED_LENGTHS, p, hist, len);
                }
            }
        }
        r = bcast(r);
        p = bcast(p);
        if (r < 0) return;
        int len = (int)r;
        long long bytePos = (p + 32) >> 3;
        if (EMIT) {
            for (int k = tid; k < len; k += NL) {
                // bytes past the end of input read as (byte)-1 in the reference (BitInputStreamUtil.readFromBIS)
                uint8_t v = (bytePos + k < sd.len) ? sd.data[bytePos + k] : 0xff;
                out.U[sd.uBase + em->uStart + k] = v;
            }
        }
        long long np = (bytePos + len) * 8;
        if (np > br.nbits) { np = br.nbits; po.eofHit = 1; }
        po.endBit = np;
        po.uLen = len;
        po.status = 0;
        return;
    }
    for (int i = tid; i < (int)(sizeof(D4GState) / 4); i += NL) ((uint32_t*)S)[i] = 0;
    __syncthreads();
    if (btype == 1) {
        // The fixed code (HuffmanTable.LIT, B/huffman/HuffmanTable.java:166-209) is the RFC 1951 code over
        // 288 symbols; 286/287 take code space but are not decodable symbols (decodeStream rejects > 285).
        for (int i = tid; i < D4G_NLIT; i += NL) S->litLen[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
        // (a diagnosis gives the codes of distance symbols 30 / 31 their lengths too, so that it can name the symbol it refuses)
        for (int i = tid; i < D4G_NDIST; i += NL) S->distLen[i] = (i < 30 || DIAG) ? 5 : 0;
        if (tid == 0) S->type = D4G_FIXED;
        __syncthreads();
    } else {
        // initDynamicDecoder — DeflateBlockHuffman.java:892-1010
        long long r = 0;
        if (tid == 0) {
            if (!br.have(14)) {
                r = -1;
                if constexpr (DIAG) diag(D4G_DIAG_EOF, br.pos(), hist, -1);
            } else {
                br.fill(L.inbuf);
                S->nLit = (int)(br.buf & 31) + 257;
                S->nDist = (int)((br.buf >> 5) & 31) + 1;
                S->nCl = (int)((br.buf >> 10) & 15) + 4;
                br.skip(14);
                if (S->nLit > 288) r = -1;
                if (strict && (S->nLit > 286 || S->nDist > 30)) r = -1;
                if (r == 0 && !br.have(3 * S->nCl)) {
                    r = -1;
                    if constexpr (DIAG) diag(D4G_DIAG_EOF, br.pos() + 3 * (br.avail() / 3), hist, -1);   // the first entry cut short
                }
                if (r == 0) {
                    for (int i = 0; i < S->nCl; i++) {
                        br.fill(L.inbuf);
                        S->clLen[D4G_CL_ORDER[i]] = (uint8_t)(br.buf & 7);
                        br.skip(3);
                    }
                }
                S->type = D4G_DYNAMIC;
                S->hdrBits = 5 + 5 + 4 + 3 * S->nCl;
            }
        }
        r = bcast(r);
        if (r < 0) return;
        d4g_build_decoder(&L.cl, S->clLen, 19);
        if (tid == 0) {
            int i = 0, np = 0;
            int combined = S->nLit + S->nDist;
            while (i < combined && r == 0) {
                br.fill(L.inbuf);
                int cl = 0, sym;
                [[maybe_unused]] const long long symPos = DIAG ? br.pos() : 0;
                D4G_DECODE(&L.cl, br.buf, br.avail(), sym, cl);
                if (sym < 0 || sym > 18) {
                    r = -1;
                    if constexpr (DIAG) {
                        int pk2;
                        diag(d4g_diag_code(&L.cl, br.buf, br.avail(), pk2) == D4G_DIAG_EOF ? D4G_DIAG_EOF : D4G_DIAG_CODE_LENGTHS, symPos, hist, -1);
                    }
                    break;
                }
                br.skip(cl);
                S->hdrBits += cl;
                int run = 0, value = sym;
                if (sym == 16) {
                    if (i < 1 || !br.have(2)) {
                        r = -1;
                        if constexpr (DIAG) {
                            if (i < 1) diag(D4G_DIAG_CODE_LENGTHS, symPos, hist, 16);
                            else diag(D4G_DIAG_EOF, br.pos(), hist, -1);
                        }
                        break;
                    }
                    run = (int)(br.buf & 3) + 3;
                    br.skip(2); S->hdrBits += 2;
                    value = (i - 1 < S->nLit) ? S->litLen[i - 1] : S->distLen[i - 1 - S->nLit];
                } else if (sym == 17) {
                    if (!br.have(3)) {
                        r = -1;
                        if constexpr (DIAG) diag(D4G_DIAG_EOF, br.pos(), hist, -1);
                        break;
                    }
                    run = (int)(br.buf & 7) + 3;
                    br.skip(3); S->hdrBits += 3;
                    value = 0;
                } else if (sym == 18) {
                    if (!br.have(7)) {
                        r = -1;
                        if constexpr (DIAG) diag(D4G_DIAG_EOF, br.pos(), hist, -1);
                        break;
                    }
                    run = (int)(br.buf & 127) + 11;
                    br.skip(7); S->hdrBits += 7;
                    value = 0;
                }
                int cnt = run ? run : 1;
                if (i + cnt > combined) {
                    r = -1;
                    if constexpr (DIAG) diag(D4G_DIAG_CODE_LENGTHS, symPos, hist, sym);
                    break;
                }
                for (int k = 0; k < cnt; k++, i++) {
                    if (i < S->nLit) S->litLen[i] = (uint8_t)value;
                    else S->distLen[i - S->nLit] = (uint8_t)value;
                }
                S->pairs[np++] = pair_encode(sym, run, value);
            }
            S->nPairs = np;
        }
        r = bcast(r);
        if (r < 0) return;
    }
    d4g_build_decoder(&L.lit, S->litLen, btype == 1 ? 288 : S->nLit);
    // (DIAG: the fixed distance table then has 32 codes and is complete, where the probe's has 30 and is not.  Whether a token
    // decodes is the same — 30 / 31 are refused as `ds > 29` instead of as "no code" — and nothing below reads L.dist.complete
    // or L.dist.nCodes unless `strict` is set, which a diagnosis never does.)
    d4g_build_decoder(&L.dist, S->distLen, btype == 1 ? (DIAG ? 32 : 30) : S->nDist);
    if (btype == 1 && tid == 0) { S->litLen[286] = 0; S->litLen[287] = 0; }
    __syncthreads();
    if (strict) {
        // speculative candidates must look like an encoder's output: complete literal/length code with an
        // EOB code, complete (or at most one-code) distance code
        bool good = L.lit.complete && S->litLen[256] > 0 && (L.dist.complete || L.dist.nCodes <= 1);
        if (!good) return;
    }
    // ---- decodeStream — DeflateBlockHuffman.java:778-890, by the whole workgroup ----
    // The block's bits are cut into chunks of D4G_CHUNK_BITS; NL (= workgroup size) chunks make a batch.  Thread i
    // decodes chunk i from a start position: thread 0 from the known token boundary, the others from a guess (their
    // chunk's first bit).  A decoder started off a token boundary usually falls into step with the true token
    // sequence after a few codes, so its exit position (first token boundary past the chunk's end) is usually
    // right.  Each pass hands every thread its left neighbour's exit as the new start and re-decodes the chunks
    // whose start changed; when a pass changes nothing, start(i+1) == exit(i) for all i and start(0) is true, so
    // every start is a true token boundary — the check is exact, at worst after NL passes.  With 512 threads a batch
    // is 32 KiB of input: most blocks are one batch, decoded by eight waves at once instead of one wave eight times.
    const long long tokensStart = bcast(br.pos());
    long long s0 = tokensStart;   // true token boundary where the batch begins
    long long G = s0;             // grid origin of the batch: chunk i covers [G + i*C, G + (i+1)*C)
    unsigned nTok = 0, nU = 0, nRef = 0, litlenBits = 0;
    int needHist = 0;
    uint2* tokOut = EMIT ? out.tok + em->tokStart : nullptr;
    uint4* refOut = EMIT ? out.refs + em->refStart : nullptr;
    uint32_t* tokRefOut = EMIT ? out.tokRef + em->tokStart : nullptr;
    const uint32_t refBase32 = EMIT ? (uint32_t)em->refStart : 0u;
    const unsigned uStart32 = EMIT ? (unsigned)em->uStart : 0u;
    long long endBit = 0;
    constexpr int C = D4G_CHUNK_BITS;
    // one chunk: mode 0 counts, mode 1 also stores the tokens (the thread's output offsets are known then), mode 2 (the
    // diagnosis) stops at the first back-reference that reaches further back than the `uAt` bytes decoded before the chunk,
    // modes 3 and 4 (the partial decode) count / store the tokens that decode to no more than `room` bytes
    [[maybe_unused]] int farPos = 0x7fffffff, farDist = 0;
    [[maybe_unused]] unsigned farU = 0;
    [[maybe_unused]] unsigned room = 0;
    auto decode_chunk = [&](auto writeTag, int start, int endc, int limRel, unsigned tokAt, unsigned uAt, unsigned refAt, int& exitp,
                            unsigned& n, unsigned& u, unsigned& r, unsigned& lb, int& need, int& fl) D4G_LAMBDA_INLINE {
        constexpr bool CAP = decltype(writeTag)::value >= 3;
        constexpr bool WRITE = decltype(writeTag)::value == 1 || decltype(writeTag)::value == 4, FAR = decltype(writeTag)::value == 2;
        int pos = start;
        n = 0; u = 0; r = 0; lb = 0; need = -0x40000000; fl = 0;
        while (pos < endc) {
            if constexpr (CAP) {
                if (u >= room) break;   // the next token is the failing one, or lies behind it
            }
            uint64_t bits = d4g_peek64(L.inbuf, pos);
            int avail = limRel - pos;
            int cl = 0, sym;
            D4G_DECODE(&L.lit, bits, avail, sym, cl);
            if (sym < 0 || sym > 285) { fl = 2; break; }
            int used = cl;
            if (sym <= 256) {
                if (WRITE) {
                    if constexpr (!CAP) atomicAdd(&S->hist[sym], 1u);
                    tokOut[tokAt + n] = make_uint2((uint32_t)sym, uStart32 + uAt + u);
                }
                n++;
                lb += (unsigned)used;
                pos += used;
                if (sym == 256) { fl = 1; break; }
                u++;
            } else {
                int eb = d4g_lsym_ebits(sym);
                int len = d4g_lsym_base(sym) + (int)((bits >> cl) & ((1u << eb) - 1));
                used += eb;
                int edge = (len == 258 && sym == 284);
                int dcl = 0, ds;
                D4G_DECODE(&L.dist, bits >> used, avail - used, ds, dcl);
                if (ds < 0 || ds > 29) { fl = 2; break; }
                int deb = d4g_dsym_ebits(ds);
                int dist = d4g_dsym_base(ds) + (int)((bits >> (used + dcl)) & ((1u << deb) - 1));
                used += dcl + deb;
                if (used > avail) { fl = 2; break; }
                if constexpr (FAR) {
                    if (dist > (int)uAt + (int)u + (int)sd.dictLen) { farPos = pos; farDist = dist; farU = u; break; }   // (a preset dictionary lies before byte 0)
                }
                if constexpr (CAP) {
                    if (u + (unsigned)len > room) break;
                }
                if (dist - (int)u > need) need = dist - (int)u;
                if (WRITE) {
                    if constexpr (!CAP) {
                        atomicAdd(&S->hist[sym], 1u);
                        atomicAdd(&S->hist[D4G_NLIT + ds], 1u);
                    }
                    tokOut[tokAt + n] = make_uint2((uint32_t)len | ((uint32_t)edge << 15) | ((uint32_t)dist << 16), uStart32 + uAt + u);
                    refOut[refAt + r] = make_uint4(d4g_ref_pack(len, sym, ds, eb + deb), uStart32 + uAt + u, 0u, 0u);
                    tokRefOut[tokAt + n] = refBase32 + refAt + r;
                }
                n++; r++;
                lb += (unsigned)used;
                pos += used;
                u += (unsigned)len;
            }
        }
        exitp = pos;
    };
    int recBatch = EMIT ? em->firstBatch : -1;   // emit: next recorded batch (its first record); probe: last recorded batch
    int firstBatch = -1;
    bool recording = !EMIT && pool.batches != nullptr;
    const bool replay = EMIT && recBatch >= 0 && pool.batches != nullptr;
    while (true) {
        uint4 rec = make_uint4(0u, 0u, 0u, 0u);
        if (replay) {   // the probe's verified starts and counts of this batch: one record per wave, nw consecutive records
            rec = pool.batches[recBatch + wave].rec[lane];
            __syncthreads();
            if (tid == 0) L.bc = (long long)rec.x;
            __syncthreads();
            s0 = tokensStart + L.bc;
        }
        // the staged input must cover the batch: NL chunks, one token of overshoot, the 12-byte window of a peek
        {
            long long baseBits = br.inBase * 8;
            bool covers = s0 >= baseBits && (G - baseBits) + (long long)NL * C + 64 + 96 <= (long long)(D4G_INCH + 16) * 8;
            if (!covers) stage(s0);   // workgroup-uniform decision
        }
        const long long baseBits = br.inBase * 8;
        const int Grel = (int)(G - baseBits), s0rel = (int)(s0 - baseBits);
        long long lim = br.nbits - baseBits;
        const int limRel = lim > 0x3fffffff ? 0x3fffffff : (int)lim;
        int start = tid == 0 ? s0rel : Grel + tid * C;
        const int endc = Grel + (tid + 1) * C;
        int exitp = start, need = 0, fl = 0;
        unsigned n = 0, u = 0, r = 0, lb = 0;
        bool dirty = true;
        if (replay) {
            start = (int)(tokensStart + (long long)rec.x - baseBits);
            n = rec.y & 1023u; r = (rec.y >> 10) & 1023u; fl = (int)(rec.y >> 20); u = rec.z; lb = rec.w;
            need = -0x40000000;   // (the host checked the distances at probe time)
        } else {
            for (int pass = 0; pass < NL + 2; pass++) {
                if (dirty) decode_chunk(std::integral_constant<int, 0>{}, start, endc, limRel, 0u, 0u, 0u, exitp, n, u, r, lb, need, fl);
                // every thread takes its left neighbour's exit (and stop flag)
                __syncthreads();
                L.xExit[tid] = exitp;
                L.xFlag[tid] = fl;
                if (tid == 0) L.anyDirty = 0;
                __syncthreads();
                const int pe = tid ? L.xExit[tid - 1] : exitp, pfl = tid ? L.xFlag[tid - 1] : fl;
                dirty = tid > 0 && pfl == 0 && pe != start;
                if (dirty) { start = pe; L.anyDirty = 1; }
                __syncthreads();
                if (!L.anyDirty) break;
            }
        }
        // the block ends (or fails) in the first thread that stopped early; threads up to it hold true tokens
        __syncthreads();
        if (tid == 0) L.firstStop = NL;
        L.xExit[tid] = exitp;
        L.xFlag[tid] = fl;
        __syncthreads();
        if (fl != 0) atomicMin(&L.firstStop, tid);
        __syncthreads();
        const int f = L.firstStop;
        const bool valid = tid <= f;
        if constexpr (!DIAG && !PART) {
            if (f < NL && L.xFlag[f] == 2) return;   // invalid code or out of input: the block does not parse
        }
        unsigned pn = valid ? n : 0u, pu = valid ? u : 0u, pr = valid ? r : 0u, plb = valid ? lb : 0u;
        unsigned sn = pn, su = pu, sr = pr;   // inclusive scans: inside the wave, then across waves
        for (int d = 1; d < 64; d <<= 1) {
            unsigned a = __shfl_up(sn, d), b = __shfl_up(su, d), c2 = __shfl_up(sr, d);
            if (lane >= d) { sn += a; su += b; sr += c2; }
        }
        const int plbw = wave_sum_i32((int)plb);
        if (lane == 63) { L.wsN[wave] = sn; L.wsU[wave] = su; L.wsR[wave] = sr; }
        if (lane == 0) L.wsB[wave] = (unsigned)plbw;
        __syncthreads();
        unsigned offN = 0, offU = 0, offR = 0, totN = 0, totU = 0, totR = 0, totB = 0;
        for (int w = 0; w < nw; w++) {
            if (w < wave) { offN += L.wsN[w]; offU += L.wsU[w]; offR += L.wsR[w]; }
            totN += L.wsN[w]; totU += L.wsU[w]; totR += L.wsR[w]; totB += L.wsB[w];
        }
        sn += offN; su += offU; sr += offR;
        {
            int nd = valid && r ? need - (int)(nU + (su - pu)) : -0x40000000;
            nd = wave_max_i32(nd);
            __syncthreads();
            if (lane == 0) L.wsM[wave] = nd;
            __syncthreads();
            for (int w = 0; w < nw; w++) if (L.wsM[w] > needHist) needHist = L.wsM[w];
        }
        if constexpr (DIAG) {
            // The first failure in token order.  Threads up to f hold true tokens (thread f: those before its invalid code) and
            // now know the bytes decoded before their chunk: a second pass finds each chunk's first back-reference that reaches
            // before the start of the stream.  The first such thread wins; without one, thread f's invalid code is the failure.
            const long long before = hist + (long long)nU + (long long)(su - pu);
            if (valid) {
                int e2, need2, fl2;
                unsigned n2, u2, r2, lb2;
                decode_chunk(std::integral_constant<int, 2>{}, start, endc, limRel, 0u, (unsigned)(before > 0x3fffffff ? 0x3fffffff : before), 0u,
                             e2, n2, u2, r2, lb2, need2, fl2);
            }
            __syncthreads();
            if (tid == 0) dg->firstFar = NL;
            __syncthreads();
            if (valid && farPos != 0x7fffffff) atomicMin(&dg->firstFar, tid);
            __syncthreads();
            const int ff = dg->firstFar;
            if (ff < NL) {
                if (tid == ff) diag(D4G_DIAG_DISTANCE_TOO_FAR, baseBits + farPos, before + farU, farDist);
                return;
            }
            if (f < NL && L.xFlag[f] == 2) {
                if (tid == f) {
                    int reason, off, value;
                    d4g_diag_token(&L.lit, &L.dist, d4g_peek64(L.inbuf, exitp), limRel - exitp, reason, off, value);
                    diag(reason, baseBits + exitp + off, before + u, value);
                }
                return;
            }
        }
        if constexpr (PART) {
            // Threads up to f hold true tokens and know the bytes decoded before their chunk.  The tokens before the failing
            // element decode to exactly `budget` bytes and the failing token adds none that fit, so every thread takes its
            // tokens while they stay within what is left of the budget: a second count, a second scan, then the stores.
            const long long before = (long long)nU + (long long)(su - pu);
            room = valid && before < budget ? (unsigned)(budget - before) : 0u;   // (budget < 2^31)
            int e2, need2, fl2;
            unsigned n2 = 0, u2 = 0, r2 = 0, lb2 = 0;
            if (room) decode_chunk(std::integral_constant<int, 3>{}, start, endc, limRel, 0u, 0u, 0u, e2, n2, u2, r2, lb2, need2, fl2);
            unsigned tn = n2, tu = u2, tr = r2;
            for (int d = 1; d < 64; d <<= 1) {
                unsigned a = __shfl_up(tn, d), b = __shfl_up(tu, d), c2 = __shfl_up(tr, d);
                if (lane >= d) { tn += a; tu += b; tr += c2; }
            }
            __syncthreads();   // (the wave totals of the first scan have been read)
            if (lane == 63) { L.wsN[wave] = tn; L.wsU[wave] = tu; L.wsR[wave] = tr; }
            __syncthreads();
            unsigned oN = 0, oR = 0, tN = 0, tU = 0, tR = 0;
            for (int w = 0; w < nw; w++) {
                if (w < wave) { oN += L.wsN[w]; oR += L.wsR[w]; }
                tN += L.wsN[w]; tU += L.wsU[w]; tR += L.wsR[w];
            }
            tn += oN; tr += oR;
            if (EMIT) {
                if ((long long)nTok + tN > capTok || (long long)nRef + tR > capRef) return;   // more than the count pass saw: write nothing (uniform)
                if (room) decode_chunk(std::integral_constant<int, 4>{}, start, endc, limRel, nTok + (tn - n2), (unsigned)before, nRef + (tr - r2), e2, n2,
                                       u2, r2, lb2, need2, fl2);
            }
            nTok += tN;
            nU += tU;
            nRef += tR;
            if (f < NL || (long long)nU >= budget) break;
            s0 = baseBits + L.xExit[NL - 1];
            G += (long long)NL * C;
            __syncthreads();   // (xExit / wave sums are rewritten by the next batch)
            continue;
        }
        if (EMIT && valid) {
            int e2, need2, fl2;
            unsigned n2, u2, r2, lb2;
            decode_chunk(std::integral_constant<int, 1>{}, start, endc, limRel, nTok + (sn - pn), nU + (su - pu), nRef + (sr - pr), e2, n2, u2, r2, lb2, need2,
                         fl2);
            if (replay) exitp = e2;
        }
        if (replay) {   // (the replayed exits were not exchanged yet)
            __syncthreads();
            L.xExit[tid] = exitp;
            __syncthreads();
        }
        if (recording) {   // leave the verified chunks to the emit pass: nw consecutive records, one per wave
            __syncthreads();
            if (tid == 0) L.bc = (long long)atomicAdd(pool.next, (unsigned)nw);
            __syncthreads();
            const unsigned idx = (unsigned)L.bc;
            if (idx + (unsigned)nw <= pool.cap) {
                D4GChunkBatch* bt = pool.batches + idx + wave;
                bt->rec[lane] = make_uint4((uint32_t)(baseBits + start - tokensStart), n | (r << 10) | ((unsigned)fl << 20), u, lb);
                if (lane == 0) bt->next = -1;
                if (tid == 0 && recBatch >= 0) pool.batches[recBatch].next = (int32_t)idx;
                if (firstBatch < 0) firstBatch = (int)idx;
                recBatch = (int)idx;
            } else {
                recording = false;   // pool exhausted: the emit pass decodes this block speculatively
                firstBatch = -2;
            }
        }
        if (replay) recBatch = pool.batches[recBatch].next;
        nTok += totN;
        nU += totU;
        nRef += totR;
        litlenBits += totB;
        if (f < NL) { endBit = baseBits + L.xExit[f]; break; }
        if (replay && recBatch < 0) return;   // (a chain that ends before the block does: cannot happen for a recorded block)
        s0 = baseBits + L.xExit[NL - 1];
        G += (long long)NL * C;
        __syncthreads();   // (xExit / wave sums are rewritten by the next batch)
    }
    __syncthreads();
    if (tid == 0) {
        S->litlenBits = (long long)litlenBits;
        S->sizeBits = S->hdrBits + (long long)litlenBits;
        S->valid = 1;
        S->maskSlot = 0;
    }
    __syncthreads();
    po.status = 0;
    po.endBit = endBit;
    po.nTok = (long long)nTok;
    po.uLen = (long long)nU;
    po.sizeBits = S->sizeBits;
    po.hdrBits = (int32_t)S->hdrBits;
    po.needHist = (long long)needHist;
    po.nRef = (int32_t)nRef;
    po.firstBatch = firstBatch == -2 ? -1 : firstBatch;
    if (EMIT && !PART) {
        D4GState* g = out.states + em->stateIdx;
        for (int i = tid; i < (int)(sizeof(D4GState) / 4); i += NL) ((uint32_t*)g)[i] = ((uint32_t*)S)[i];
    }
}

// With `hits` set, only the candidates that parse are reported, compacted (the scan's candidates are mostly
// false positives; the host reads back a few hundred records instead of all of them).
struct D4GProbeHit { D4GProbeIn in; D4GProbeOut out; };
__global__ void __launch_bounds__(D4G_PARSE_MAXTHREADS) k_probe_blocks(const D4GStreamDesc* streams, const D4GProbeIn* in, D4GProbeOut* outp, unsigned n,
                                                     D4GProbeHit* hits, unsigned* nHits, D4GChunkPool pool) {
    if (blockIdx.x >= n) return;
    const D4GProbeIn pi = in[blockIdx.x];
    D4GProbeOut po;
    D4GParseOut none = {nullptr, nullptr, nullptr, nullptr, nullptr};
    d4g_parse_block<false>(streams[pi.stream], pi.bitPos, pi.strict, po, nullptr, none, pool);
    if (threadIdx.x == 0) {
        if (hits) {
            if (po.status == 0) {
                unsigned k = atomicAdd(nHits, 1u);
                hits[k].in = pi;
                hits[k].out = po;
            }
        } else {
            outp[blockIdx.x] = po;
        }
    }
}

// Diagnosis: one workgroup per stream whose parse failed decodes the failing block once more and reports the first failure
// in token order.  Launched only when a caller asks why (d4g_batch_parse_error); nothing on the parse path runs it.
__global__ void __launch_bounds__(D4G_PARSE_MAXTHREADS) k_diagnose_blocks(const D4GStreamDesc* streams, const D4GDiagIn* in, D4GDiagOut* outp) {
    __shared__ D4GDiagRec rec;
    const D4GDiagIn di = in[blockIdx.x];
    if (threadIdx.x == 0) { rec.reason = D4G_DIAG_OK; rec.firstFar = 0; rec.bitPos = -1; rec.decoded = -1; rec.value = -1; }
    __syncthreads();
    D4GProbeOut po;
    D4GParseOut none = {nullptr, nullptr, nullptr, nullptr, nullptr};
    d4g_parse_block<false, true>(streams[di.stream], di.bitPos, 0, po, nullptr, none, D4GChunkPool{nullptr, nullptr, 0u}, &rec, di.hist);
    __syncthreads();
    if (threadIdx.x == 0) {
        D4GDiagOut o;
        o.reason = rec.reason; o.pad = 0; o.bitPos = rec.bitPos; o.decoded = rec.decoded; o.value = rec.value;
        outp[blockIdx.x] = o;
    }
}

// Emit: one wave per block decodes it again, now writing tokens, back-reference records, the block's
// initial state (stored blocks: their bytes).
__global__ void __launch_bounds__(D4G_PARSE_MAXTHREADS) k_emit_blocks(const D4GStreamDesc* streams, const D4GEmitIn* in, D4GParseOut out, int32_t* errors,
                                                    D4GChunkPool pool) {
    const D4GEmitIn em = in[blockIdx.x];
    D4GProbeOut po;
    d4g_parse_block<true>(streams[em.stream], em.bitPos, 0, po, &em, out, pool);
    if (threadIdx.x == 0 && (po.status != 0 || po.uLen != em.uLen)) atomicAdd(errors, 1);
}

// Recovery (d4g_batch_recover): the block that did not parse, decoded up to the failure the diagnosis found.  One workgroup
// per block; the count pass sizes the token arrays, the emit pass fills them like k_emit_blocks does for a whole block.
struct D4GRecoverIn {
    D4GEmitIn em;          // count pass: stream and bitPos only
    long long budget;      // bytes the block's tokens before the failing element decode to
    long long nTok, nRef;  // emit pass: what the count pass found
};
__global__ void __launch_bounds__(D4G_PARSE_MAXTHREADS) k_recover_count(const D4GStreamDesc* streams, const D4GRecoverIn* in, D4GProbeOut* outp) {
    const D4GRecoverIn ri = in[blockIdx.x];
    D4GProbeOut po;
    D4GParseOut none = {nullptr, nullptr, nullptr, nullptr, nullptr};
    d4g_parse_block<false, false, true>(streams[ri.em.stream], ri.em.bitPos, 0, po, nullptr, none, D4GChunkPool{nullptr, nullptr, 0u}, nullptr, 0, ri.budget);
    if (threadIdx.x == 0) outp[blockIdx.x] = po;
}
__global__ void __launch_bounds__(D4G_PARSE_MAXTHREADS) k_recover_emit(const D4GStreamDesc* streams, const D4GRecoverIn* in, D4GParseOut out, int32_t* errors) {
    const D4GRecoverIn ri = in[blockIdx.x];
    D4GProbeOut po;
    d4g_parse_block<true, false, true>(streams[ri.em.stream], ri.em.bitPos, 0, po, &ri.em, out, D4GChunkPool{nullptr, nullptr, 0u}, nullptr, 0, ri.budget,
                                       ri.nTok, ri.nRef);
    if (threadIdx.x == 0 && (po.status != 0 || po.uLen != ri.budget || po.nTok != ri.nTok || po.nRef != ri.nRef)) atomicAdd(errors, 1);
}

// ---------------------------------------------------------------------------------------
// 4. Decoded bytes by pointer jumping.  src[q] (u32, stream-relative) is the position byte q
// copies from; literals and stored bytes point at themselves.
// ---------------------------------------------------------------------------------------
struct D4GTokRange { int32_t stream; int32_t stored; long long tokStart, tokCount, uStart, uLen; };
// An entry whose top bit is set is final: the position in its low 31 bits holds the byte itself (a literal, a stored byte).
// Final entries are never looked up again — by the last rounds that is most of them.  (A stream decodes to less than 2 GiB.)
#define D4G_SRC_FINAL 0x80000000u

__global__ void __launch_bounds__(256) k_fill_src(const D4GStreamDesc* streams, const D4GTokRange* ranges, const uint2* tok,
                                                  uint8_t* U, uint32_t* src, int32_t* badDist, int G) {
    const D4GTokRange r = ranges[blockIdx.x / G];
    const D4GStreamDesc sd = streams[r.stream];
    uint32_t* s = src + sd.uBase;
    uint8_t* u = U + sd.uBase;
    const uint32_t dictLen = (uint32_t)sd.dictLen;
    long long stride = (long long)G * blockDim.x;
    long long t0 = (long long)(blockIdx.x % G) * blockDim.x + threadIdx.x;
    if (r.stored) {
        for (long long k = t0; k < r.uLen; k += stride) s[r.uStart + k] = (uint32_t)(r.uStart + k) | D4G_SRC_FINAL;
        return;
    }
    for (long long t = t0; t < r.tokCount; t += stride) {
        uint2 tk = tok[r.tokStart + t];
        uint32_t a = tk.x, pos = tk.y;
        int dist = tok_dist(a), val = tok_val(a);
        if (dist == 0) {
            if (val < 256) { u[pos] = (uint8_t)val; s[pos] = pos | D4G_SRC_FINAL; }
        } else if ((uint32_t)dist > pos + dictLen) {
            badDist[r.stream] = 1;  // reference: readSlice walks off the first block (NullPointerException)
            for (int k = 0; k < val; k++) s[pos + k] = (pos + k) | D4G_SRC_FINAL;
        } else if ((uint32_t)dist > pos) {
            // the copy begins in the preset dictionary: those bytes are known now and become literals; what follows (the copy
            // may run on into the stream's own bytes, and overlap itself) points back as any copy does
            const int inDict = (int)((uint32_t)dist - pos) < val ? (int)((uint32_t)dist - pos) : val;
            for (int k = 0; k < inDict; k++) { u[pos + k] = sd.dict[dictLen + pos + k - (uint32_t)dist]; s[pos + k] = (pos + k) | D4G_SRC_FINAL; }
            for (int k = inDict; k < val; k++) s[pos + k] = pos + k - dist;
        } else {
            for (int k = 0; k < val; k++) s[pos + k] = pos + k - dist;
        }
    }
}

// One stream per blockIdx.y.  In place: reading a concurrently updated entry still yields an ancestor.
// `prev` (the previous round's moved-entries counter, nullptr for the first round): the rounds of a batch are launched
// back to back and a round whose predecessor moved fewer than stopNum entries does nothing — the host reads the counters
// once per batch instead of once per round.
__global__ void __launch_bounds__(256) k_jump_streams(const D4GStreamDesc* streams, uint32_t* src, unsigned long long* changed, int G,
                                                      const unsigned long long* prev, unsigned long long stopNum) {
    if (prev && *prev < stopNum) return;
    const D4GStreamDesc sd = streams[blockIdx.x / G];
    uint32_t* s = src + sd.uBase;   // uBase is a multiple of 16: four entries per 16-byte load
    const long long n4 = sd.uLen >> 2;
    long long stride = (long long)G * blockDim.x;
    int any = 0;   // entries this thread moved
    // four consecutive entries per thread and step: one coalesced 16-byte load, four gathers in flight
    for (long long q4 = (long long)(blockIdx.x % G) * blockDim.x + threadIdx.x; q4 < n4; q4 += stride) {
        const uint32_t q = (uint32_t)(q4 << 2);
        uint4 a = *(const uint4*)(s + q);
        uint32_t b0 = (a.x & D4G_SRC_FINAL) ? a.x : s[a.x], b1 = (a.y & D4G_SRC_FINAL) ? a.y : s[a.y];
        uint32_t b2 = (a.z & D4G_SRC_FINAL) ? a.z : s[a.z], b3 = (a.w & D4G_SRC_FINAL) ? a.w : s[a.w];
        bool c0 = b0 != a.x, c1 = b1 != a.y, c2 = b2 != a.z, c3 = b3 != a.w;
        if (c0 | c1 | c2 | c3) {
            *(uint4*)(s + q) = make_uint4(b0, b1, b2, b3);
            any += (int)c0 + (int)c1 + (int)c2 + (int)c3;
        }
    }
    if (blockIdx.x % G == 0 && threadIdx.x < (sd.uLen & 3)) {   // the last one to three entries
        long long q = (n4 << 2) + threadIdx.x;
        uint32_t a = s[q];
        uint32_t b = (a & D4G_SRC_FINAL) ? a : s[a];
        if (b != a) { s[q] = b; any++; }
    }
    // how many entries moved this round (the host stops doubling once few do; k_resolve_streams walks the rest);
    // one global atomic per workgroup
    __shared__ unsigned wgMoved;
    if (threadIdx.x == 0) wgMoved = 0;
    __syncthreads();
    int tot = wave_sum_i32(any);
    if (tot && (threadIdx.x & 63) == 0) atomicAdd(&wgMoved, (unsigned)tot);
    __syncthreads();
    if (threadIdx.x == 0 && wgMoved) atomicAdd((unsigned long long*)changed, (unsigned long long)wgMoved);
}
// The first doubling rounds, tile by tile.  A round's gathers reach 32 KiB * 2^round back: for the first few rounds that is the
// tile itself and a handful of tiles before it.  One workgroup owns one 32 Ki-entry tile and runs `reps` rounds over it in a
// row while its neighbours (same XCD: consecutive tiles get workgroup ids that are equal mod 8) do the same to theirs, so the
// entries and their targets are served by that XCD's L2 after the first touch instead of crossing to HBM every round — as far as
// the tiles in flight fit: the launch is 1024 threads per tile and asks for 70 KiB of (unused) LDS, two tiles per CU at most.  In
// place and unsynchronised like k_jump_streams: any value read is a position further up the same copy chain.
#define D4G_JUMP_TILE 32768
struct D4GJumpTile { int32_t stream, pad; long long first; };
__global__ void __launch_bounds__(1024) k_jump_tiles(const D4GStreamDesc* streams, const D4GJumpTile* tiles, uint32_t* src, int reps,
                                                    unsigned long long* changed) {
    // (the launch asks for LDS it does not use — d4g_host.h: that bounds the workgroups per CU, so that the tiles in flight stay in L2)
    const D4GJumpTile t = tiles[blockIdx.x];
    const D4GStreamDesc sd = streams[t.stream];
    uint32_t* s = src + sd.uBase;
    const long long q0 = t.first, q1 = q0 + D4G_JUMP_TILE < sd.uLen ? q0 + D4G_JUMP_TILE : sd.uLen;
    const long long n4 = (q1 - q0) >> 2;
    int any = 0;
    for (int rep = 0; rep < reps; rep++) {
        any = 0;
        for (long long k = threadIdx.x; k < n4; k += blockDim.x) {
            const long long q = q0 + (k << 2);
            uint4 a = *(const uint4*)(s + q);
            uint32_t b0 = (a.x & D4G_SRC_FINAL) ? a.x : s[a.x], b1 = (a.y & D4G_SRC_FINAL) ? a.y : s[a.y];
            uint32_t b2 = (a.z & D4G_SRC_FINAL) ? a.z : s[a.z], b3 = (a.w & D4G_SRC_FINAL) ? a.w : s[a.w];
            bool c0 = b0 != a.x, c1 = b1 != a.y, c2 = b2 != a.z, c3 = b3 != a.w;
            if (c0 | c1 | c2 | c3) {
                *(uint4*)(s + q) = make_uint4(b0, b1, b2, b3);
                any += (int)c0 + (int)c1 + (int)c2 + (int)c3;
            }
        }
        if ((long long)threadIdx.x < ((q1 - q0) & 3)) {   // the last one to three entries of the stream
            const long long q = q0 + (n4 << 2) + threadIdx.x;
            uint32_t a = s[q];
            uint32_t b = (a & D4G_SRC_FINAL) ? a : s[a];
            if (b != a) { s[q] = b; any++; }
        }
    }
    __shared__ unsigned wgMoved;
    if (threadIdx.x == 0) wgMoved = 0;
    __syncthreads();
    int tot = wave_sum_i32(any);
    if (tot && (threadIdx.x & 63) == 0) atomicAdd(&wgMoved, (unsigned)tot);
    __syncthreads();
    if (threadIdx.x == 0 && wgMoved) atomicAdd((unsigned long long*)changed, (unsigned long long)wgMoved);
}
__global__ void __launch_bounds__(256) k_resolve_streams(const D4GStreamDesc* streams, const uint32_t* src, uint8_t* U, int G) {
    const D4GStreamDesc sd = streams[blockIdx.x / G];
    const uint32_t* s = src + sd.uBase;
    uint8_t* u = U + sd.uBase;
    long long stride = (long long)G * blockDim.x;
    for (long long q = (long long)(blockIdx.x % G) * blockDim.x + threadIdx.x; q < sd.uLen; q += stride) {
        uint32_t a = s[q];
        if (a != ((uint32_t)q | D4G_SRC_FINAL)) {
            // (pointer doubling stops early: follow what is left of the chain — every hop lands further up it)
            while (!(a & D4G_SRC_FINAL)) a = s[a];
            u[q] = u[a & ~D4G_SRC_FINAL];
        }
    }
}

// ---------------------------------------------------------------------------------------
// 4b. Decoded bytes block by block, with window markers (D4G_COPY=blocks; the two-pass scheme of pugz / rapidgzip).
// A DEFLATE distance is at most 32 768, so a copy reads what its own segment produced or one of the 32 768 bytes
// before the segment: a segment (one block, or a run of small blocks of one stream) decodes in one ordered pass
// without knowing what precedes it.  What it cannot know becomes a marker into that window.
//   k_seg_symbols      one workgroup per segment: 16-bit symbols (a byte, or D4G_SYM_MARK | i = byte i of the window)
//                      for every decoded byte, and the segment's last 32 Ki symbols (its "tail": a map from the window
//                      before the segment to the window after it);
//   k_seg_compose      tails compose: a logarithmic scan over the segments of a stream resolves every window;
//   k_seg_substitute   every byte reads its symbol, markers are looked up in the segment's resolved window, U is
//                      written once.
// No chain is followed across the stream and no count comes back to the host.
// ---------------------------------------------------------------------------------------
#define D4G_WIN 32768
#define D4G_SEG_GROUP_BYTES 4096    // decoded bytes one group of tokens may produce (what the ring holds beyond the window)
#define D4G_SEG_GROUP_TOKENS 511    // tokens per group (one more is staged for its position: the end of the group)
#define D4G_SEG_RING (D4G_WIN + D4G_SEG_GROUP_BYTES)
#define D4G_SYM_MARK 0x8000u        // | i: byte i of the 32 KiB before the segment
#define D4G_SYM_PTR 0x4000u         // inside a group only: | offset of the byte of the same group this one copies
static_assert(((D4G_SEG_GROUP_TOKENS + 1) & D4G_SEG_GROUP_TOKENS) == 0, "the token search takes power-of-two steps");
static_assert(D4G_SEG_GROUP_BYTES <= 0x4000 && D4G_SEG_GROUP_BYTES >= 258, "a group offset fits a pointer symbol; any token fits a group");
struct D4GSegment {
    int32_t stream;
    int32_t rangeFirst, rangeCount;   // its blocks (D4GTokRange records, consecutive)
    int32_t tail;                     // slot its tail is written to (-1: nobody needs it)
    int32_t win;                      // slot that holds its resolved window after the scan (-1: first segment of its stream)
    int32_t pad;
    long long uStart, uLen;           // stream-relative decoded range
};
#define D4G_SUB_CHUNK 65536         // decoded bytes one workgroup of the substitution pass writes
struct D4GSubChunk { int32_t stream, win; long long first, count; };
struct D4GSegLds {
    uint16_t ring[D4G_SEG_RING];      // symbol of segment-relative position j (j >= -32768) at slot (j + 32768) % D4G_SEG_RING
    uint32_t pos[D4G_SEG_GROUP_TOKENS + 1];
    uint32_t a[D4G_SEG_GROUP_TOKENS + 1];
    int n;
    int anyPtr[3];
};

// One group at a time: up to 511 tokens that produce up to 4096 bytes.  Every byte of the group finds its token (binary
// search over the staged positions) and becomes the literal, the finished symbol of its source (a source before the group
// is final), or a pointer to its source inside the group; pointer doubling in LDS then resolves the group in at most
// log2(4096) rounds whatever the tokens are — a run of tokens that each depend on the one before (PNG rows at distance
// 3-4, long runs) costs rounds, not one round per token.
// DICT: some stream of the batch has a preset dictionary.  A batch without one runs the instantiation that knows of none: the
// code of the default path is what it was before dictionaries.
template <bool DICT>
__global__ void __launch_bounds__(1024) k_seg_symbols(const D4GStreamDesc* streams, const D4GSegment* segs, const D4GTokRange* ranges,
                                                                      const uint2* tok, const uint8_t* U, uint16_t* sym, uint16_t* tails,
                                                                      int32_t* badDist) {
    __shared__ D4GSegLds L;
    const int tid = threadIdx.x, NL = blockDim.x;
    const D4GSegment sg = segs[blockIdx.x];
    const D4GStreamDesc sd = streams[sg.stream];
    uint16_t* out = sym + sd.uBase + sg.uStart;
    const uint32_t segStart = (uint32_t)sg.uStart;
    // The window before the segment is unknown: markers.  Before a stream's first segment lies its preset dictionary, if it has
    // one: those bytes are known, the window's last dictLen symbols; the markers left in front of them are the positions too far back.
    const uint32_t dictLen = DICT ? (uint32_t)sd.dictLen : 0u;
    if constexpr (DICT) {
        const int known = sg.win < 0 ? D4G_WIN - (int)dictLen : D4G_WIN;   // window symbols from here on are dictionary bytes
        for (int i = tid; i < D4G_WIN; i += NL) L.ring[i] = i >= known ? (uint16_t)sd.dict[i - known] : (uint16_t)(D4G_SYM_MARK | (uint32_t)i);
    } else {
        for (int i = tid; i < D4G_WIN; i += NL) L.ring[i] = (uint16_t)(D4G_SYM_MARK | (uint32_t)i);
    }
    if (tid == 0) { L.n = D4G_SEG_GROUP_TOKENS; L.anyPtr[0] = 0; L.anyPtr[1] = 0; L.anyPtr[2] = 0; }
    __syncthreads();
    int rr = 0;   // doubling rounds so far (workgroup-uniform): round r raises anyPtr[r % 3]
    bool bad = false;
    for (int r = 0; r < sg.rangeCount; r++) {
        const D4GTokRange rg = ranges[sg.rangeFirst + r];
        const uint32_t b0 = (uint32_t)(rg.uStart - sg.uStart), bLen = (uint32_t)rg.uLen;
        if (rg.stored) {   // the emit pass has put the bytes into U
            const uint8_t* u = U + sd.uBase + rg.uStart;
            for (uint32_t k = tid; k < bLen; k += NL) {
                const uint16_t v = u[k];
                if (bLen - k <= D4G_WIN) L.ring[(b0 + k + D4G_WIN) % D4G_SEG_RING] = v;   // (what a later copy can reach)
                out[b0 + k] = v;
            }
            __syncthreads();
            continue;
        }
        const uint2* tk = tok + rg.tokStart;
        long long t0 = 0;
        uint32_t gs = b0;
        uint2 pre = make_uint2(0u, 0u);
        if (tid < rg.tokCount) pre = tk[tid];
        while (t0 < rg.tokCount) {
            const long long left = rg.tokCount - t0;
            const int m = left < D4G_SEG_GROUP_TOKENS ? (int)left : D4G_SEG_GROUP_TOKENS, m1 = left < D4G_SEG_GROUP_TOKENS + 1 ? (int)left : D4G_SEG_GROUP_TOKENS + 1;
            // stage the tokens; the group ends before the first one whose bytes would pass the group's byte bound
            for (int i = tid; i <= D4G_SEG_GROUP_TOKENS; i += NL) {
                if (i >= m1) { L.pos[i] = 0xffffffffu; continue; }   // (the search below may look at any staged slot)
                const uint2 t = i == tid ? pre : tk[t0 + i];
                const uint32_t p = t.y - segStart;
                const int dist = tok_dist(t.x), val = tok_val(t.x);
                const uint32_t len = dist ? (uint32_t)val : (val < 256 ? 1u : 0u);
                L.pos[i] = p;
                L.a[i] = t.x;
                if (i < m && p + len - gs > D4G_SEG_GROUP_BYTES) atomicMin(&L.n, i);
            }
            __syncthreads();
            const int n = L.n < m ? L.n : m;
            const uint32_t ge = n < m1 ? L.pos[n] : b0 + bLen;
            if (t0 + n + tid < rg.tokCount) pre = tk[t0 + n + tid];   // the next group's tokens, asked for now
            // K bytes per thread side by side: the LDS reads of a step are independent of each other and overlap
            constexpr int K = 4;
            for (uint32_t base = gs + tid; base < ge; base += K * NL) {
                uint32_t j[K], e[K];
                int lo[K];
#pragma unroll
                for (int k = 0; k < K; k++) { j[k] = base + k * NL; lo[k] = 0; }
                // the last token that starts at or before j (an end-of-block token has no bytes and is last): tokens from n on
                // start at or after the group's end, the slots past the staged ones hold the largest position
#pragma unroll
                for (int st = (D4G_SEG_GROUP_TOKENS + 1) / 2; st > 0; st >>= 1) {
#pragma unroll
                    for (int k = 0; k < K; k++)
                        if (L.pos[lo[k] + st] <= j[k]) lo[k] += st;
                }
#pragma unroll
                for (int k = 0; k < K; k++) {
                    const bool in = j[k] < ge;
                    const uint32_t a = L.a[in ? lo[k] : 0];
                    const uint32_t dist = in ? (uint32_t)tok_dist(a) : 0u;
                    const uint32_t back = L.ring[(j[k] + D4G_WIN - dist) % D4G_SEG_RING];   // (final if it lies before the group, unused otherwise)
                    if (!dist) e[k] = a & 0xffu;
                    else if (dist > segStart + j[k] + dictLen) { e[k] = 0; bad = true; }   // before the start of the stream (and of its dictionary)
                    else if (j[k] - gs >= dist) e[k] = D4G_SYM_PTR | (j[k] - dist - gs);
                    else e[k] = back;
                }
#pragma unroll
                for (int k = 0; k < K; k++)
                    if (j[k] < ge) L.ring[(j[k] + D4G_WIN) % D4G_SEG_RING] = (uint16_t)e[k];
            }
            __syncthreads();
            if (tid == 0) L.n = D4G_SEG_GROUP_TOKENS;
            // in place and unsynchronised, like k_jump_streams: any value read is further up the same chain, or final
            for (;;) {
                bool mine = false;
                for (uint32_t base = gs + tid; base < ge; base += K * NL) {
                    uint32_t e[K], e2[K];
#pragma unroll
                    for (int k = 0; k < K; k++) e[k] = base + k * NL < ge ? L.ring[(base + k * NL + D4G_WIN) % D4G_SEG_RING] : 0u;
#pragma unroll
                    for (int k = 0; k < K; k++) e2[k] = L.ring[(gs + (e[k] & 0x3fffu) + D4G_WIN) % D4G_SEG_RING];
#pragma unroll
                    for (int k = 0; k < K; k++)
                        if ((e[k] & 0xc000u) == D4G_SYM_PTR) {
                            L.ring[(base + k * NL + D4G_WIN) % D4G_SEG_RING] = (uint16_t)e2[k];
                            mine |= (e2[k] & 0xc000u) == D4G_SYM_PTR;
                        }
                }
                if (mine) L.anyPtr[rr % 3] = 1;
                if (tid == 0) L.anyPtr[(rr + 1) % 3] = 0;   // (last read two barriers ago)
                __syncthreads();
                const int any = L.anyPtr[rr % 3];
                rr++;
                if (!any) break;
            }
            for (uint32_t j = gs + tid; j < ge; j += NL) out[j] = L.ring[(j + D4G_WIN) % D4G_SEG_RING];
            gs = ge;
            t0 += n;
        }
        __syncthreads();   // (a stored block that follows rewrites most of the ring)
    }
    if (bad) badDist[sg.stream] = 1;  // reference: readSlice walks off the first block (NullPointerException)
    if (sg.tail >= 0) {
        __syncthreads();
        uint16_t* t = tails + (long long)sg.tail * D4G_WIN;
        const uint32_t q0 = (uint32_t)sg.uLen;
        for (int i = tid; i < D4G_WIN; i += NL) t[i] = L.ring[(q0 + (uint32_t)i) % D4G_SEG_RING];
    }
}

// One round of the scan over tail slots (the slots of a stream are consecutive; ord = index inside the stream): slot s
// takes the markers of its map through the map of slot s - d.  Ping-pong, not in place: `out` is complete after the round.
__global__ void __launch_bounds__(256) k_seg_compose(const int32_t* slotOrd, const uint16_t* in, uint16_t* out, int d, int G) {
    const long long slot = blockIdx.x / G;
    const bool look = slotOrd[slot] >= d;
    const uint4* a = (const uint4*)(in + slot * D4G_WIN);
    uint4* o = (uint4*)(out + slot * D4G_WIN);
    const uint16_t* prev = in + (slot - (look ? d : 0)) * D4G_WIN;
    auto via = [&](uint32_t w) D4G_LAMBDA_INLINE {   // two symbols
        uint32_t lo = w & 0xffffu, hi = w >> 16;
        if (lo & D4G_SYM_MARK) lo = prev[lo & 0x7fffu];
        if (hi & D4G_SYM_MARK) hi = prev[hi & 0x7fffu];
        return lo | (hi << 16);
    };
    for (int i = (blockIdx.x % G) * blockDim.x + threadIdx.x; i < D4G_WIN / 8; i += G * blockDim.x) {
        uint4 v = a[i];
        if (look && ((v.x | v.y | v.z | v.w) & 0x80008000u)) v = make_uint4(via(v.x), via(v.y), via(v.z), via(v.w));
        o[i] = v;
    }
}

__global__ void __launch_bounds__(1024) k_seg_substitute(const D4GStreamDesc* streams, const D4GSubChunk* chunks, const uint16_t* sym,
                                                        const uint16_t* tails, uint8_t* U) {
    alignas(16) __shared__ uint8_t W[D4G_WIN];
    const D4GSubChunk c = chunks[blockIdx.x];
    const D4GStreamDesc sd = streams[c.stream];
    const int tid = threadIdx.x, NL = blockDim.x;
    const bool hasWin = c.win >= 0;
    auto low2 = [](uint32_t w) D4G_LAMBDA_INLINE { return (w & 0xffu) | ((w >> 8) & 0xff00u); };   // the low bytes of two symbols
    if (hasWin) {
        // (a marker left in a resolved window points before the start of the stream: only a stream with a bad distance has one)
        const uint4* t = (const uint4*)(tails + (long long)c.win * D4G_WIN);
        for (int i = tid; i < D4G_WIN / 8; i += NL) {
            const uint4 v = t[i];
            *(uint2*)(W + i * 8) = make_uint2(low2(v.x) | (low2(v.y) << 16), low2(v.z) | (low2(v.w) << 16));
        }
        __syncthreads();
    }
    const uint16_t* s = sym + sd.uBase;
    uint8_t* u = U + sd.uBase;
    auto res = [&](uint32_t h) D4G_LAMBDA_INLINE -> uint32_t { return (hasWin && (h & D4G_SYM_MARK)) ? W[h & 0x7fffu] : (h & 0xffu); };
    auto res2 = [&](uint32_t w) D4G_LAMBDA_INLINE -> uint32_t { return res(w & 0xffffu) | (res(w >> 16) << 8); };
    const long long a = c.first, b = c.first + c.count;
    long long a8 = (a + 7) & ~7LL, b8 = b & ~7LL;
    if (a8 > b) a8 = b;
    if (b8 < a8) b8 = a8;
    for (long long q = a + tid; q < a8; q += NL) u[q] = (uint8_t)res(s[q]);
    for (long long q = a8 + (long long)tid * 8; q < b8; q += (long long)NL * 8) {   // uBase is a multiple of 16: aligned 16-byte loads, 8-byte stores
        const uint4 v = *(const uint4*)(s + q);
        uint2 w;
        if ((v.x | v.y | v.z | v.w) & 0x80008000u) w = make_uint2(res2(v.x) | (res2(v.y) << 16), res2(v.z) | (res2(v.w) << 16));
        else w = make_uint2(low2(v.x) | (low2(v.y) << 16), low2(v.z) | (low2(v.w) << 16));
        *(uint2*)(u + q) = w;
    }
    for (long long q = b8 + tid; q < b; q += NL) u[q] = (uint8_t)res(s[q]);
}

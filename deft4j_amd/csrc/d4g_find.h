// d4g_find.h — kernels of d4g_find_streams: where, in a file of unknown layout, do zlib and gzip streams begin?
//   k_find_wrappers   one thread per byte offset tests the two wrapper headers (include/deft4g.h states the predicates)
//   k_find_confirm    one thread per decoded candidate compares the checksums of its decoded bytes with its trailer
// Everything between the two — trial parse, decode, checksums — is the ordinary parse path (d4g_parse.h, d4g_write.h),
// sequenced by d4g_host_find.h.
#pragma once
#include "d4g_parse.h"
#include "d4g_write.h"

#define D4G_FOUND_KIND_ZLIB 1   // = D4G_FOUND_ZLIB / D4G_FOUND_GZIP of the C ABI
#define D4G_FOUND_KIND_GZIP 2
// kind: D4G_FOUND_KIND_* in the low byte; a zlib header with FDICT carries 1 + the index of its preset dictionary above it
struct D4GFindCand { int32_t file, kind; long long offset, payload; };
#define D4G_FIND_KIND(k) ((k) & 0xff)
#define D4G_FIND_DICT(k) (((k) >> 8) - 1)   // -1: none
struct D4GScanTile { int32_t stream; int32_t pad; long long byteStart; };   // one workgroup's bytes of a file
#define D4G_FIND_TILE 2048
#define D4G_FIND_LOCAL 64   // candidates a workgroup collects before it touches the global list (random bytes give about one per tile)

// The gzip member header at byte o of a file (the 10 fixed bytes are inside it and say gzip): the first byte after the
// optional fields in RFC 1952 order, -1 when one of them does not end inside the file.
D4G_DEV long long d4g_gzip_payload(const uint8_t* data, long long len, long long o, int flg) {
    long long p = o + 10;
    if (flg & 4) {   // FEXTRA
        if (p + 2 > len) return -1;
        p += 2 + ((long long)data[p] | ((long long)data[p + 1] << 8));
        if (p > len) return -1;
    }
    for (int f = 8; f <= 16; f <<= 1) {   // FNAME, FCOMMENT: zero-terminated
        if (!(flg & f)) continue;
        while (p < len && data[p] != 0) p++;
        if (p >= len) return -1;
        p++;
    }
    if (flg & 2) p += 2;   // FHCRC: skipped, not checked
    return p <= len ? p : -1;
}

// One thread per byte offset, the tile staged in LDS as k_scan_headers stages its own.  Candidates are collected per
// workgroup and take one global atomic per tile (an atomic per hit on one counter is far slower); a tile with more than
// D4G_FIND_LOCAL of them sends the rest straight to the global list.  The count may pass `cap`: the host then runs the
// kernel again with a list that holds them all.
// dictIds: the Adler-32 of each of the caller's nDict preset dictionaries (d4g_find_streams_dict): a zlib header with FDICT
// whose DICTID is one of them is a candidate too, the first match in list order, its payload 4 bytes further on.
__global__ void __launch_bounds__(256) k_find_wrappers(const D4GStreamDesc* files, const D4GScanTile* tiles, int kinds, D4GFindCand* cands,
                                                       unsigned* nCands, unsigned cap, const uint32_t* dictIds, int nDict) {
    alignas(16) __shared__ uint8_t buf[D4G_FIND_TILE + 16];
    __shared__ D4GFindCand lc[D4G_FIND_LOCAL];
    __shared__ unsigned lcount, gbase;
    if (threadIdx.x == 0) lcount = 0;
    const D4GScanTile tile = tiles[blockIdx.x];
    const D4GStreamDesc sd = files[tile.stream];
    for (int i = threadIdx.x * 16; i < D4G_FIND_TILE + 16; i += blockDim.x * 16)
        *(uint4*)(buf + i) = *(const uint4*)(sd.data + tile.byteStart + i);  // the input buffer is padded past len
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (int b = threadIdx.x; b < D4G_FIND_TILE; b += blockDim.x) {   // (the same trip count for every thread: the ballot below)
        const long long o = tile.byteStart + b;
        const int c0 = buf[b], c1 = buf[b + 1];
        D4GFindCand c;
        c.file = tile.stream; c.kind = 0; c.offset = o; c.payload = -1;
        if ((kinds & (1 << D4G_FOUND_KIND_ZLIB)) && o + 2 <= sd.len && (c0 & 15) == 8 && (c0 >> 4) <= 7 && ((c0 << 8) + c1) % 31 == 0 &&
            !(c1 & 0x20)) {
            c.kind = D4G_FOUND_KIND_ZLIB;
            c.payload = o + 2;
        } else if (nDict && (kinds & (1 << D4G_FOUND_KIND_ZLIB)) && o + 6 <= sd.len && (c0 & 15) == 8 && (c0 >> 4) <= 7 &&
                   ((c0 << 8) + c1) % 31 == 0) {   // FDICT: DICTID, big-endian, right after FLG
            const uint32_t id = ((uint32_t)buf[b + 2] << 24) | ((uint32_t)buf[b + 3] << 16) | ((uint32_t)buf[b + 4] << 8) | (uint32_t)buf[b + 5];
            for (int d = 0; d < nDict; d++)
                if (dictIds[d] == id) {
                    c.kind = D4G_FOUND_KIND_ZLIB | ((d + 1) << 8);
                    c.payload = o + 6;
                    break;
                }
        } else if ((kinds & (1 << D4G_FOUND_KIND_GZIP)) && o + 10 <= sd.len && c0 == 0x1f && c1 == 0x8b && buf[b + 2] == 8 && !(buf[b + 3] & 0xe0)) {
            c.kind = D4G_FOUND_KIND_GZIP;
            c.payload = d4g_gzip_payload(sd.data, sd.len, o, buf[b + 3]);   // (rare: the optional fields are read where they lie)
        }
        const bool ok = c.payload >= 0;
        unsigned long long m = __ballot(ok);
        if (m) {
            unsigned base = 0;
            if (lane == 0) base = atomicAdd(&lcount, (unsigned)__popcll(m));
            base = __shfl(base, 0);
            if (ok) {
                unsigned idx = base + (unsigned)__popcll(m & ((1ULL << lane) - 1));
                if (idx < D4G_FIND_LOCAL) lc[idx] = c;
                else {
                    unsigned g = atomicAdd(nCands, 1u);
                    if (g < cap) cands[g] = c;
                }
            }
        }
    }
    __syncthreads();
    const unsigned nl = lcount < D4G_FIND_LOCAL ? lcount : D4G_FIND_LOCAL;
    if (threadIdx.x == 0) gbase = nl ? atomicAdd(nCands, nl) : 0u;
    __syncthreads();
    for (unsigned i = threadIdx.x; i < nl; i += blockDim.x)
        if (gbase + i < cap) cands[gbase + i] = lc[i];
}

// One thread per decoded candidate: its trailer where it lies in the file (zlib: Adler-32, big-endian; gzip: CRC-32 then
// ISIZE, little-endian) against the checksums of its decoded bytes.
struct D4GFindCheck { const uint8_t* trailer; int32_t kind, pad; };
struct D4GFindVerdict { uint32_t crc32, adler32; int32_t ok, pad; };
__global__ void __launch_bounds__(64) k_find_confirm(const D4GFindCheck* in, const D4GCsumOut* sums, unsigned n, D4GFindVerdict* out) {
    const unsigned k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const D4GFindCheck c = in[k];
    const D4GCsumOut s = sums[k];
    const uint8_t* t = c.trailer;
    bool ok;
    if (c.kind == D4G_FOUND_KIND_ZLIB) {
        ok = (((uint32_t)t[0] << 24) | ((uint32_t)t[1] << 16) | ((uint32_t)t[2] << 8) | (uint32_t)t[3]) == s.adler32;
    } else {
        const uint32_t crc = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
        const uint32_t isize = (uint32_t)t[4] | ((uint32_t)t[5] << 8) | ((uint32_t)t[6] << 16) | ((uint32_t)t[7] << 24);
        ok = crc == s.crc32 && isize == (uint32_t)s.isize;
    }
    D4GFindVerdict v;
    v.crc32 = s.crc32; v.adler32 = s.adler32; v.ok = ok ? 1 : 0; v.pad = 0;
    out[k] = v;
}

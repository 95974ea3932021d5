// d4g_host_find.h — sequencing of d4g_find_streams: wrapper headers at every byte offset, a trial parse of the survivors
// as block chains over the files' shared header map, decode + checksum + trailer compare of the chains that parse.
// Every file is uploaded once and scanned once; a candidate is a chain start at bit payload_offset * 8 of its file, never
// a stream of its own over the rest of the file.  Decoded bytes stay in device memory.
#pragma once
#include "d4g_find.h"

namespace d4g {

#define D4G_FIND_GROUP_STREAMS 512        // candidates decoded together: at most this many,
#define D4G_FIND_GROUP_BYTES (256LL << 20)   // and (beyond the first) no more decoded bytes than this

struct FindRun {
    std::vector<d4g_found_stream> found;   // sorted by (file, offset)
    d4g_find_stats st;
    double msKernels = 0;

    // k_find_wrappers over every file -> the candidates in (file, offset) order
    std::vector<D4GFindCand> wrappers(Batch& F, int kinds, const std::vector<uint32_t>& dictIds) {
        std::vector<D4GScanTile> tiles;
        i64 total = 0;
        for (size_t i = 0; i < F.streams.size(); i++) {
            for (i64 b = 0; b < F.streams[i].inLen; b += D4G_FIND_TILE) tiles.push_back({(int32_t)i, 0, b});
            total += F.streams[i].inLen;
        }
        std::vector<D4GFindCand> cands;
        if (tiles.empty()) return cands;
        RtScratch tmp;
        D4GScanTile* dTiles = tmp.upload(tiles);
        unsigned* dN = tmp.alloc<unsigned>(1);
        const uint32_t* dIds = dictIds.empty() ? nullptr : tmp.upload(dictIds);
        unsigned cap = (unsigned)std::max<i64>(4096, total / 256), nc = 0;
        for (int attempt = 0; attempt < 2; attempt++) {
            D4GFindCand* dC = tmp.alloc<D4GFindCand>((size_t)cap);
            rt_memset(dN, 0, 4);
            RT_LAUNCH(k_find_wrappers, tiles.size(), 256, F.dStreams, dTiles, kinds, dC, dN, cap, dIds, (int)dictIds.size());
            st.kernel_launches++;
            rt_d2h(&nc, dN, 4);
            if (nc <= cap) {
                cands.resize(nc);
                rt_d2h(cands.data(), dC, (size_t)nc * sizeof(D4GFindCand));
                break;
            }
            cap = nc;
        }
        tmp.release();
        std::sort(cands.begin(), cands.end(), [](const D4GFindCand& a, const D4GFindCand& b) {
            return a.file != b.file ? a.file < b.file : a.offset < b.offset;
        });
        return cands;
    }

    // One group of parsed candidates: decode (emit + copy path), checksums, trailer compare.  The group is a batch whose
    // streams are the candidates' chains over their files' bytes, which it borrows from F for as long as it lives.
    std::vector<D4GFindVerdict> confirm(Batch& F, const std::vector<D4GFindCand>& cands, const std::vector<Batch::PStream>& chains,
                                        const std::vector<size_t>& group) {
        const size_t m = group.size();
        struct Borrow {   // the files' bytes go back to F on every way out
            Batch& F; Batch& G;
            Borrow(Batch& F, Batch& G) : F(F), G(G) { G.dIn = std::move(F.dIn); }
            ~Borrow() { try { rt_sync_all(); } catch (...) {} F.dIn = std::move(G.dIn); }
        };
        Batch G;
        memset(&G.stats, 0, sizeof(G.stats));
        Borrow borrow(F, G);
        G.streams.resize(m);
        G.ps.resize(m);
        std::vector<D4GFindCheck> checks(m);
        for (size_t k = 0; k < m; k++) {
            const D4GFindCand& c = cands[group[k]];
            G.streams[k].inOff = F.streams[c.file].inOff;
            G.streams[k].inLen = F.streams[c.file].inLen;
            if (const int d = D4G_FIND_DICT(c.kind); d >= 0 && F.dictTail[d]) { G.streams[k].dict = F.dDict + F.dictOff[d]; G.streams[k].dictLen = F.dictTail[d]; }
            G.ps[k] = chains[group[k]];
            for (Batch::PBlock& pb : G.ps[k].blocks) pb.firstBatch = -1;   // (the scan's chunk records went back with the scan)
            checks[k] = {G.dIn + G.streams[k].inOff + G.ps[k].consumed, D4G_FIND_KIND(c.kind), 0};
        }
        G.build_blocks(false, false);
        RtScratch tmp;
        RtEvent e0, e1;
        e0.record();
        D4GCsumOut* dSums = G.launch_checksums(tmp);
        D4GFindCheck* dChecks = tmp.upload(checks);
        D4GFindVerdict* dV = tmp.alloc<D4GFindVerdict>(m);
        RT_LAUNCH(k_find_confirm, (m + 63) / 64, 64, dChecks, dSums, (unsigned)m, dV);
        G.stats.kernel_launches++;
        e1.record();
        std::vector<D4GFindVerdict> v(m);
        rt_d2h(v.data(), dV, m * sizeof(D4GFindVerdict));
        tmp.release();
        msKernels += G.msParseKernels + rt_elapsed_ms(e0, e1);
        st.kernel_launches += G.stats.kernel_launches;
        return v;
    }

    // RFC 1950's Adler-32 of a whole dictionary: its DICTID
    static uint32_t adler32(const uint8_t* p, size_t n) {
        uint32_t a = 1, b = 0;
        while (n) {
            const size_t k = std::min<size_t>(n, 5552);   // (the sums stay below 2^32 for this many bytes)
            for (size_t i = 0; i < k; i++) { a += p[i]; b += a; }
            a %= 65521; b %= 65521;
            p += k; n -= k;
        }
        return (b << 16) | a;
    }

    void run(size_t n, const uint8_t* const* file, const size_t* len, int kinds, i64 minDecoded, size_t nDict = 0, const uint8_t* const* dict = nullptr,
             const size_t* dictLen = nullptr) {
        const double t0 = now_ms();
        memset(&st, 0, sizeof(st));
        if (kinds == 0) kinds = (1 << D4G_FOUND_KIND_ZLIB) | (1 << D4G_FOUND_KIND_GZIP);
        engine().init();
        Batch F;
        F.create(n, file, len);
        std::vector<uint32_t> dictIds(nDict);
        for (size_t d = 0; d < nDict; d++) dictIds[d] = adler32(dict[d], dictLen[d]);
        if (nDict) F.set_dictionaries(nDict, dict, dictLen, nullptr);   // (the tails: a candidate names its dictionary)
        auto dict_len_of = [&](const D4GFindCand& c) { return D4G_FIND_DICT(c.kind) >= 0 ? F.dictTail[D4G_FIND_DICT(c.kind)] : (i64)0; };
        st.bytes_scanned = F.stats.bytes_in;
        // 1. every file's dynamic-header map (once), the wrapper candidates, and their trial parse: the first block of
        //    every candidate, then the whole chain of the survivors
        RtEvent e0, e1;
        e0.record();
        Batch::BlockMap M;
        F.scan_inputs(M);
        const std::vector<D4GFindCand> all = wrappers(F, kinds, dictIds);
        st.header_candidates = (i64)all.size();
        std::vector<Batch::ChainStart> starts(all.size());
        for (size_t k = 0; k < all.size(); k++) starts[k] = {all[k].file, all[k].payload * 8, dict_len_of(all[k])};
        std::vector<Batch::PStream> first;
        F.walk_chains(starts, M, first, 1);
        std::vector<D4GFindCand> cands;
        starts.clear();
        for (size_t k = 0; k < all.size(); k++)
            if (first[k].status == 0) { cands.push_back(all[k]); starts.push_back({all[k].file, all[k].payload * 8, dict_len_of(all[k])}); }
        st.first_block_ok = (i64)cands.size();
        std::vector<Batch::PStream> chains;
        F.walk_chains(starts, M, chains, 0);
        e1.record();
        msKernels += rt_elapsed_ms(e0, e1);
        F.dChunkBatches.reset(); F.dChunkNext.reset();
        F.chunkPool = {nullptr, nullptr, 0};
        // 2. the chains that parsed, with their trailer inside the file and enough decoded bytes, in (file, offset) order
        std::vector<size_t> todo;
        for (size_t k = 0; k < cands.size(); k++) {
            if (chains[k].status != 0) continue;
            st.parsed++;
            const i64 trailer = D4G_FIND_KIND(cands[k].kind) == D4G_FOUND_KIND_ZLIB ? 4 : 8;
            if (chains[k].consumed + trailer > F.streams[cands[k].file].inLen || chains[k].nU < minDecoded) continue;
            todo.push_back(k);
        }
        // 3. groups of bounded size; a candidate that starts inside a stream already reported is dropped before it is
        //    decoded, one inside a stream of its own group after it
        std::vector<i64> reportedEnd(n, 0);
        for (size_t at = 0; at < todo.size();) {
            std::vector<size_t> group;
            i64 bytes = 0;
            for (; at < todo.size(); at++) {
                const size_t k = todo[at];
                if (cands[k].offset < reportedEnd[cands[k].file]) continue;
                if (!group.empty() && (group.size() >= D4G_FIND_GROUP_STREAMS || bytes + chains[k].nU > D4G_FIND_GROUP_BYTES)) break;
                group.push_back(k);
                bytes += chains[k].nU;
            }
            if (group.empty()) break;
            const std::vector<D4GFindVerdict> v = confirm(F, cands, chains, group);
            for (size_t q = 0; q < group.size(); q++) {
                if (!v[q].ok) continue;
                st.confirmed++;
                const D4GFindCand& c = cands[group[q]];
                const Batch::PStream& P = chains[group[q]];
                if (c.offset < reportedEnd[c.file]) continue;
                d4g_found_stream f;
                memset(&f, 0, sizeof(f));
                f.file = c.file; f.kind = D4G_FIND_KIND(c.kind); f.dictionary = D4G_FIND_DICT(c.kind) + 1; f.offset = c.offset; f.payload_offset = c.payload;
                f.payload_len = P.consumed - c.payload;
                f.total_len = P.consumed + (f.kind == D4G_FOUND_KIND_ZLIB ? 4 : 8) - c.offset;
                f.decoded_len = P.nU; f.size_bits = P.sizeBits;
                f.crc32 = v[q].crc32; f.adler32 = v[q].adler32;
                f.n_blocks = (int32_t)P.blocks.size();
                found.push_back(f);
                reportedEnd[c.file] = c.offset + f.total_len;
            }
        }
        st.reported = (i64)found.size();
        st.kernel_launches += F.stats.kernel_launches;
        st.ms_kernels = msKernels;
        rt_sync_all();
        st.ms_total = now_ms() - t0;
    }
};

}  // namespace d4g

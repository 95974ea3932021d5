// d4g_lz77_host.h — host sequencing of the LZ77 front end (d4g_lz77.h): a batch whose streams are produced by the
// zlib-level-9-compatible encoder kernels instead of parsed from compressed input.  The encoder leaves tokens,
// back-reference records, decoded bytes (= the raw input) and one D4GState per block in exactly the layout the parser
// produces, so DeflateStream.optimise / mergeBlocks / write (d4g_host.h) run on them unchanged — the reference's
// `compressor.compress(data)` followed by `Deft.optimiseDeflateStream(out)` (C/CompressorTask.java:29-35) without
// serialising and re-parsing the intermediate stream.
#pragma once
#include <string>
#include <tuple>

#include "d4g_host.h"
#include "d4g_lz77.h"

namespace d4g {

struct LzSpec { int32_t input, encoder, strategy; };   // mirrors d4g_encoder_spec (include/deft4g.h)
struct LzSpecL { int32_t input, encoder, strategy, level; };   // mirrors d4g_encoder_spec_level; LzSpec = level 9

// zlib 1.2.11's configuration_table (deflate.c): good_length, max_lazy (deflate_fast: max_insert_length), nice_length,
// max_chain; levels 1-3 run deflate_fast, 4-9 deflate_slow
struct LzLevelCfg { int good, lazy, nice, chain; };
inline LzLevelCfg lz_level_cfg(int level) {
    static const LzLevelCfg t[10] = {{0, 0, 0, 0},     {4, 4, 8, 4},       {4, 5, 16, 8},       {4, 6, 32, 32},     {4, 4, 16, 16},
                                     {8, 16, 32, 32},  {8, 16, 128, 128},  {8, 32, 128, 256},   {32, 128, 258, 1024}, {32, 258, 258, 4096}};
    return t[level];
}

// the parse a spec needs, as a key: specs with equal keys share one parse of their input.  kind -1: none (HUFFMAN_ONLY).
struct LzParseKey {
    int input, kind, strategy, level;
    bool operator<(const LzParseKey& o) const {
        return std::tie(input, kind, strategy, level) < std::tie(o.input, o.kind, o.strategy, o.level);
    }
};
inline LzParseKey lz_parse_key(const LzSpecL& s) {
    if (s.strategy == LZ_HUFFMAN_ONLY) return {s.input, -1, 0, 0};
    if (s.strategy == LZ_RLE) return {s.input, LZ_KIND_RLE, 0, 0};
    if (s.level <= 3) return {s.input, LZ_KIND_FAST, 0, s.level};   // deflate_fast ignores FILTERED
    return {s.input, LZ_KIND_SLOW, s.strategy == LZ_FILTERED ? LZ_FILTERED : LZ_DEFAULT, s.level};   // FIXED parses as DEFAULT
}

// why a spec with a level is refused ("" = accepted); level -1 is zlib's Z_DEFAULT_COMPRESSION (6)
inline std::string lz_spec_refusal(const LzSpecL& s, size_t nIn) {
    if (s.input < 0 || (size_t)s.input >= nIn) return "encoder spec: input out of range";
    if (s.encoder < 0 || s.encoder > 1) return "encoder spec: unknown encoder";
    if (s.strategy < 0 || s.strategy > LZ_FIXED) return "encoder spec: unknown strategy";
    if (s.level == 0) return "encoder spec: level 0 is not supported (zlib's deflate_stored output depends on the caller's output buffer)";
    if (s.level < -1 || s.level > 9) return "encoder spec: level must be -1 or 1..9";
    if (s.encoder == LZ_FLAVOR_JZLIB && (s.level != 9 || s.strategy > LZ_HUFFMAN_ONLY))
        return "encoder spec: the jzlib flavour supports level 9 with DEFAULT / FILTERED / HUFFMAN_ONLY only";
    return "";
}

// Preset dictionaries (deflateSetDictionary, zlib 1.2.11): the tail that counts is the last w_size = 32768 bytes, and a
// dictionary of length 0 is none.  dictOf: per input an index, or -1.
inline i64 lz_dict_tail(size_t nDict, const size_t* dictLen, const int32_t* dictOf, size_t input) {
    if (!nDict || !dictOf || dictOf[input] < 0) return 0;
    return (i64)std::min<size_t>(dictLen[dictOf[input]], LZ_SORT_BLOCK);
}
// why specs are refused next to these dictionaries ("" = accepted; the specs have passed lz_spec_refusal)
inline std::string lz_dict_spec_refusal(size_t nOut, const LzSpecL* sp, size_t nDict, const size_t* dictLen, const int32_t* dictOf) {
    for (size_t i = 0; i < nOut; i++)
        if (sp[i].encoder == LZ_FLAVOR_JZLIB && lz_dict_tail(nDict, dictLen, dictOf, (size_t)sp[i].input) > 0)
            return "encoder spec: the jzlib flavour takes no preset dictionary (jzlib's setDictionary follows an older zlib rule — a 32506-byte tail, "
                   "the last two strings never inserted — that nothing here can pin)";
    return "";
}

struct LzFront {
    Batch& B;
    std::vector<LzSpecL> specs;   // levels resolved (-1 -> 6)
    std::vector<i64> rawLen, rawU;   // per input: its length and where its first byte lies in dU (16-byte aligned)
    std::vector<i64> dictTail;       // per input: bytes of dictionary tail that lie in dU right before it (0: none)
    explicit LzFront(Batch& b) : B(b) {}
    // input i where it lies in dU: stable from create() on, whatever runs on the batch
    DevBytes input(size_t i) const { return {B.dU + rawU[i], (size_t)rawLen[i]}; }

    // the specs of the level-9 entry points (DEFAULT / FILTERED / HUFFMAN_ONLY only) as specs with a level
    static std::vector<LzSpecL> at_level_9(size_t nIn, size_t nOut, const LzSpec* sp) {
        for (size_t i = 0; i < nOut; i++)
            if (sp[i].input < 0 || (size_t)sp[i].input >= nIn || sp[i].encoder < 0 || sp[i].encoder > 1 || sp[i].strategy < 0 || sp[i].strategy > 2)
                throw std::runtime_error("bad encoder spec");
        std::vector<LzSpecL> l(nOut);
        for (size_t i = 0; i < nOut; i++) l[i] = {sp[i].input, sp[i].encoder, sp[i].strategy, 9};
        return l;
    }
    // dict / dictLen / dictOf (host memory; the caller has checked them — dict_refusal and lz_dict_spec_refusal, libdeft4g.hip): per input that names a
    // dictionary, dU holds [tail of the dictionary][input] contiguously, padded IN FRONT of the tail so that the input
    // stays 16-byte aligned (the optimiser, the writer and the checksums load it so); the encoder kernels read the tail
    // bytewise or through the aligned-down window staging.  The output streams carry that copy as their HStream::dict.
    void create(size_t nIn, const uint8_t* const* raw, const size_t* len, size_t nOut, const LzSpecL* sp, bool fromDevice = false, size_t nDict = 0,
                const uint8_t* const* dict = nullptr, const size_t* dictLen = nullptr, const int32_t* dictOf = nullptr) {
        memset(&B.stats, 0, sizeof(B.stats));
        double t0 = now_ms();
        specs.assign(sp, sp + nOut);
        for (LzSpecL& s : specs) {
            const std::string why = lz_spec_refusal(s, nIn);
            if (!why.empty()) throw std::runtime_error(why);
            if (s.level == -1) s.level = 6;
        }
        rawLen.resize(nIn);
        rawU.resize(nIn);
        dictTail.resize(nIn);
        i64 off = 0;
        for (size_t i = 0; i < nIn; i++) {
            dictTail[i] = lz_dict_tail(nDict, dictLen, dictOf, i);
            if ((i64)len[i] + dictTail[i] >= 0x7fff0000LL) throw std::runtime_error("input of 2 GiB or more: split it");
            rawLen[i] = (i64)len[i];
            rawU[i] = off + ((dictTail[i] + 15) & ~15LL);
            off = rawU[i] + (((i64)len[i] + 15) & ~15LL) + 512;   // zero padding: the kernels read (never use) a few words past the end
            B.stats.bytes_decoded += (i64)len[i];
            B.stats.dict_bytes += dictTail[i];
        }
        B.dU.alloc_zero((size_t)off, 1024);
        for (size_t i = 0; i < nIn; i++) {
            if (fromDevice) rt_d2d(B.dU + rawU[i], raw[i], len[i]);
            else rt_h2d(B.dU + rawU[i], raw[i], len[i]);
            if (dictTail[i]) {
                const size_t d = (size_t)dictOf[i];
                rt_h2d(B.dU + rawU[i] - dictTail[i], dict[d] + (dictLen[d] - (size_t)dictTail[i]), (size_t)dictTail[i]);
            }
        }
        rt_sync();
        B.streams.resize(nOut);
        for (size_t o = 0; o < nOut; o++) {
            const i64 t = dictTail[specs[o].input];
            if (!t) continue;
            B.streams[o].dict = B.dU + rawU[specs[o].input] - t;
            B.streams[o].dictLen = t;
            B.stats.dict_streams++;
        }
        B.stats.n_streams = (i64)nOut;
        B.stats.ms_upload = now_ms() - t0;
    }

    // The whole front end: fills B.ps / B.streams / the device arrays, then runs the batch's own phases.
    void run(bool optimise, bool merge) {
        if (B.ran) throw std::runtime_error("batch already ran");
        B.ran = true;
        Engine& E = engine();
        E.init();
        double t0 = now_ms();
        const size_t nIn = rawLen.size(), nOut = specs.size();
        // ---- 1. streams, sort blocks, chunks ----
        std::vector<LzStream> hs(nIn);
        std::vector<LzSortJob> sortJobs;
        i64 posTot = 0;
        for (size_t i = 0; i < nIn; i++) {
            // positions, chunks and sort blocks are those of tail(dictionary) || input (d4g_lz77.h, "Coordinates")
            hs[i].data = B.dU + rawU[i] - dictTail[i];
            hs[i].len = dictTail[i] + rawLen[i];
            hs[i].dictLen = dictTail[i];
            hs[i].posBase = posTot;
            hs[i].sortBlock0 = (int32_t)(posTot / LZ_SORT_BLOCK);
            hs[i].nChunks = (int32_t)((hs[i].len + LZ_CHUNK - 1) / LZ_CHUNK);
            i64 nsb = rawLen[i] > 0 ? (hs[i].len + LZ_SORT_BLOCK - 1) / LZ_SORT_BLOCK : 0;   // (an empty input is never sorted, dictionary or not)
            posTot += nsb * LZ_SORT_BLOCK;
        }
        auto first_chunk = [&](int input) { return (int)(dictTail[input] / LZ_CHUNK); };   // the chunk that holds the input's first byte
        // parses needed: one per (input, effective parse) — lz_parse_key; HUFFMAN_ONLY needs neither sort nor parse, and
        // deflate_rle no sort.  deflate_fast parses also get an insertion map (LZ_CHUNK_WORDS words per chunk).
        std::map<LzParseKey, int> parseOf;
        struct Parse { int input, kind, strategy, level; i64 metaBase, insBase; };
        std::vector<Parse> parses;
        std::vector<char> needSort(nIn, 0);
        i64 metaTot = 0, insTot = 0;
        for (const LzSpecL& s : specs) {
            const LzParseKey key = lz_parse_key(s);
            if (key.kind < 0 || parseOf.count(key)) continue;
            parseOf[key] = (int)parses.size();
            parses.push_back({key.input, key.kind, key.strategy, key.level, metaTot, key.kind == LZ_KIND_FAST ? insTot : -1});
            metaTot += hs[s.input].nChunks;
            if (key.kind == LZ_KIND_FAST) insTot += (i64)hs[s.input].nChunks * LZ_CHUNK_WORDS;
            if (key.kind != LZ_KIND_RLE && rawLen[s.input] > 0) needSort[s.input] = 1;   // (an empty input behind a dictionary: nothing is searched)
        }
        for (size_t i = 0; i < nIn; i++)
            if (needSort[i])
                for (i64 b = 0; b * LZ_SORT_BLOCK < hs[i].len; b++) sortJobs.push_back({(int32_t)i, (int32_t)b});
        // device buffers of the front end that must not outlive it: released before the batch's own phases start
        RtScratch tmp;
        LzStream* dStreamsLz = tmp.alloc<LzStream>(nIn, 16);
        rt_h2d(dStreamsLz, hs.data(), nIn * sizeof(LzStream));
        uint16_t *dS16 = nullptr, *dRank = nullptr, *dBstart = nullptr;
        LzChunkMeta* dMeta = nullptr;
        uint32_t* dChunkTok = nullptr;
        std::vector<LzChunkMeta> meta((size_t)metaTot);
        RtEvent e0, e1, e2;
        e0.record();
        if (!sortJobs.empty()) {
            dS16 = tmp.alloc<uint16_t>((size_t)posTot, 64);
            dRank = tmp.alloc<uint16_t>((size_t)posTot, 64);
            dBstart = tmp.alloc<uint16_t>((size_t)posTot, 64);   // 32768 entries per sort block
            RtScratch st;
            LzSortJob* dJobs = st.upload(sortJobs);
            RT_LAUNCH(k_lz_sort, sortJobs.size(), LZ_SORT_THREADS, dStreamsLz, dJobs, dS16, dRank, dBstart);
            B.stats.kernel_launches++;
            rt_sync();
            st.release();
        }
        e1.record();
        // ---- 2. parse: speculative pass over every chunk, then exact re-runs until entry == predecessor's exit ----
        LzCtx c;
        c.streams = dStreamsLz; c.S16 = dS16; c.rank16 = dRank; c.bstart = dBstart; c.errors = B.errors();
        c.meta = nullptr; c.chunkTok = nullptr; c.insLive = nullptr; c.insFrozen = nullptr; c.insChg = nullptr;
        if (metaTot > 0) {
            dMeta = tmp.alloc<LzChunkMeta>((size_t)metaTot);
            dChunkTok = tmp.alloc<uint32_t>((size_t)metaTot * (LZ_CHUNK + 2), 64);
            c.meta = dMeta; c.chunkTok = dChunkTok;
            uint8_t* dFast = nullptr;
            if (insTot > 0) {
                c.insLive = tmp.alloc<uint32_t>((size_t)insTot, 64);
                c.insFrozen = tmp.alloc<uint32_t>((size_t)insTot, 64);
                c.insChg = tmp.alloc<int32_t>((size_t)metaTot, 16);
                rt_memset(c.insLive, 0xff, (size_t)insTot * 4);   // a chunk that has not run yet: "every position inserted"
                rt_memset(c.insChg, 0xff, (size_t)metaTot * 4);   // -1: never changed
                dFast = tmp.alloc<uint8_t>((size_t)metaTot, 16);
            }
            auto makeJob = [&](const Parse& P, int firstChunk) {
                const LzLevelCfg g = lz_level_cfg(P.kind == LZ_KIND_RLE ? 9 : P.level);
                return LzParseJob{P.input, firstChunk, (int32_t)P.metaBase, P.strategy, g.good, g.lazy, g.nice, g.chain, P.insBase};
            };
            // one launch per parse kind (each its own kernel); the jobs are grouped by kind
            auto launch = [&](std::vector<LzParseJob>& jobs, const std::vector<int>& kindOf, int exact, const uint8_t* dHeadsArg, int pass,
                              LzParseJob* dJobs) {
                std::vector<LzParseJob> sorted;
                size_t cnt[3] = {0, 0, 0};
                for (int k = 0; k < 3; k++)
                    for (size_t j = 0; j < jobs.size(); j++)
                        if (kindOf[j] == k) { sorted.push_back(jobs[j]); cnt[k]++; }
                rt_h2d(dJobs, sorted.data(), sorted.size() * sizeof(LzParseJob));
                const unsigned threads = exact ? 64 : 64 * LZ_PARSE_MAXWAVES;
                size_t off = 0;
                if (cnt[LZ_KIND_SLOW]) { RT_LAUNCH(k_lz_parse<LZ_KIND_SLOW>, cnt[0], threads, c, dJobs + off, exact, dHeadsArg, pass); B.stats.kernel_launches++; }
                off += cnt[0];
                if (cnt[LZ_KIND_FAST]) { RT_LAUNCH(k_lz_parse<LZ_KIND_FAST>, cnt[1], threads, c, dJobs + off, exact, dHeadsArg, pass); B.stats.kernel_launches++; }
                off += cnt[1];
                if (cnt[LZ_KIND_RLE]) { RT_LAUNCH(k_lz_parse<LZ_KIND_RLE>, cnt[2], threads, c, dJobs + off, exact, dHeadsArg, pass); B.stats.kernel_launches++; }
            };
            std::vector<LzParseJob> jobs;
            std::vector<int> jobKind;
            std::vector<int32_t> chunkIndex((size_t)metaTot), chunkParse((size_t)metaTot);
            std::vector<uint8_t> chunkFast((size_t)metaTot, 0);
            for (size_t pi = 0; pi < parses.size(); pi++) {
                const Parse& P = parses[pi];
                // (the chunks before the input's first byte lie wholly in the dictionary: nothing to parse)
                for (int fc = first_chunk(P.input); fc < hs[P.input].nChunks; fc += LZ_PARSE_MAXWAVES) { jobs.push_back(makeJob(P, fc)); jobKind.push_back(P.kind); }
                for (int k = 0; k < hs[P.input].nChunks; k++) {
                    chunkIndex[P.metaBase + k] = k; chunkParse[P.metaBase + k] = (int32_t)pi;
                    chunkFast[P.metaBase + k] = P.kind == LZ_KIND_FAST;
                }
            }
            // Dictionary chunks record no tokens and hand the first parsed chunk its exact start: entry = exit =
            // lz_pack_state(dictLen, 0, 2, 0), so k_lz_check's induction begins at the chunk that holds dictLen.  (An
            // input that ends where its dictionary does has no such chunk, or one that finds nothing to do.)  Only these
            // metas are the host's; every other chunk is launched and writes its own.
            for (const Parse& P : parses) {
                const int nd = std::min(first_chunk(P.input), (int)hs[P.input].nChunks);
                if (nd == 0) continue;
                LzChunkMeta m;
                memset(&m, 0, sizeof(m));
                m.entry = m.exit = lz_pack_state(dictTail[P.input], 0, 2, 0);
                m.firstPos = (uint32_t)dictTail[P.input];
                std::vector<LzChunkMeta> init((size_t)nd, m);
                for (int k = 0; k < nd; k++) init[k].chainStart = k;
                rt_h2d(dMeta + P.metaBase, init.data(), init.size() * sizeof(LzChunkMeta));
            }
            if (dFast) rt_h2d(dFast, chunkFast.data(), (size_t)metaTot);
            RtScratch st;
            LzParseJob* dJobs = st.alloc<LzParseJob>(std::max(jobs.size(), (size_t)metaTot), 16);
            launch(jobs, jobKind, 0, nullptr, 0, dJobs);
            B.stats.lz_parse_passes = 1;
            int32_t* dIdx = tmp.alloc<int32_t>((size_t)metaTot, 16);
            int32_t* dRedo = tmp.alloc<int32_t>((size_t)metaTot, 16);
            uint8_t* dHeads = tmp.alloc<uint8_t>((size_t)metaTot, 16);
            unsigned* dN = tmp.alloc<unsigned>(4);
            rt_h2d(dIdx, chunkIndex.data(), (size_t)metaTot * 4);
            std::vector<uint8_t> heads((size_t)metaTot);
            for (int pass = 1;; pass++) {
                if (pass > 100000) throw std::runtime_error("lz77 parse did not converge");
                rt_memset(dN, 0, 4);
                RT_LAUNCH(k_lz_check, (metaTot + 255) / 256, 256, dMeta, dIdx, (int)metaTot, dRedo, dN, (const uint8_t*)dFast, (const int32_t*)c.insChg);
                B.stats.kernel_launches++;
                unsigned nr = 0;
                rt_d2h(&nr, dN, 4);
                if (nr == 0) break;
                std::vector<int32_t> redo(nr);
                rt_d2h(redo.data(), dRedo, (size_t)nr * 4);
                // A run of consecutive disagreeing chunks is one job: its first chunk (the head) is re-run from its
                // predecessor's exit and the wave carries on through the run — and beyond, while exits keep differing
                // from recorded entries — until it falls into step or reaches another job's head.  In the first exact
                // pass a deflate_fast chunk stale only through insertion bits (bit 31) starts a job of its own: after
                // the speculative pass nearly every chunk is, and each needs only its predecessors' first-pass bits.
                // Later, chains of dependent chunks converge faster as one wave than one chunk per pass.
                std::fill(heads.begin(), heads.end(), 0);
                std::vector<char> bad((size_t)metaTot, 0);
                for (unsigned k = 0; k < nr; k++) bad[redo[k] & 0x7fffffff] = 1;
                std::vector<LzParseJob> rj;
                std::vector<int> rjKind;
                for (unsigned k = 0; k < nr; k++) {
                    const int m = redo[k] & 0x7fffffff;
                    const bool bitsOnly = redo[k] < 0;
                    if (chunkIndex[m] > 0 && bad[m - 1] && !(bitsOnly && pass == 1)) continue;   // inside a run: the run's head gets there
                    const Parse& P = parses[chunkParse[m]];
                    rj.push_back(makeJob(P, chunkIndex[m]));
                    rjKind.push_back(P.kind);
                    heads[m] = 1;
                }
                rt_h2d(dHeads, heads.data(), (size_t)metaTot);
                if (insTot > 0) rt_d2d((void*)c.insFrozen, c.insLive, (size_t)insTot * 4);   // what this pass's runs read
                launch(rj, rjKind, 1, dHeads, pass, dJobs);
                B.stats.lz_parse_passes++;
                B.stats.lz_chunks_rerun += nr;
            }
            rt_d2h(meta.data(), dMeta, (size_t)metaTot * sizeof(LzChunkMeta));
            st.release();
        }
        e2.record();
        B.check_device_errors();
        // ---- 3. output streams: symbol counts, block boundaries, array bases ----
        std::vector<LzOutStream> outs(nOut);
        std::vector<LzBlockDesc> blocks;
        std::vector<LzFillJob> fillJobs;
        i64 tokTot = 0, refTot = 0;
        std::vector<i64> outSyms(nOut), outRefs(nOut);
        std::vector<std::vector<i64>> symPreOf(nOut), refPreOf(nOut);
        std::vector<char> lastIsMatchOf(nOut, 0);
        std::vector<int> kindOf(nOut, -1);
        // jzlib flavour: its early-flush decisions need prefix sums at symbol granularity -> k_lz_split
        std::vector<LzSplitJob> splitJobs;
        std::vector<size_t> splitOut;
        std::vector<i64> preSym, preRef, preDc;
        i64 splitSlots = 0;
        for (size_t oi = 0; oi < nOut; oi++) {
            const LzSpecL& sp = specs[oi];
            const LzStream& st = hs[sp.input];
            LzOutStream& o = outs[oi];
            o.stream = sp.input;
            o.metaBase = -1;
            std::vector<i64>&symPre = symPreOf[oi], &refPre = refPreOf[oi];
            symPre.assign(st.nChunks + 1, 0);
            refPre.assign(st.nChunks + 1, 0);
            std::vector<i64> dcPre(st.nChunks + 1, 0);
            bool lastIsMatch = false;
            const LzParseKey pk = lz_parse_key(sp);
            o.flags = (sp.strategy == LZ_FIXED ? LZ_OUT_FIXED : 0) | (pk.kind == LZ_KIND_FAST || pk.kind == LZ_KIND_RLE ? LZ_OUT_TOP_AT_TOKEN : 0) |
                      (pk.kind == LZ_KIND_RLE ? LZ_OUT_RLE_FILL : 0);
            kindOf[oi] = pk.kind;
            if (pk.kind >= 0) {
                const Parse& P = parses[parseOf[pk]];
                o.metaBase = (int32_t)P.metaBase;
                for (int k = 0; k < st.nChunks; k++) {
                    const LzChunkMeta& m = meta[P.metaBase + k];
                    symPre[k + 1] = symPre[k] + m.ntok;
                    refPre[k + 1] = refPre[k] + m.nmatch;
                    dcPre[k + 1] = dcPre[k] + m.dcost;
                    if (m.ntok) lastIsMatch = (m.pad >> 9) != 0;
                }
            } else {
                for (int k = 0; k < st.nChunks; k++) symPre[k + 1] = std::max<i64>(0, std::min<i64>(st.len, (i64)(k + 1) * LZ_CHUNK) - st.dictLen);
            }
            lastIsMatchOf[oi] = lastIsMatch;
            outSyms[oi] = symPre[st.nChunks];
            outRefs[oi] = refPre[st.nChunks];
            if (sp.encoder == LZ_FLAVOR_JZLIB) {
                LzSplitJob J;
                memset(&J, 0, sizeof(J));
                J.stream = sp.input; J.metaBase = o.metaBase; J.preBase = (i64)preSym.size();
                J.nSyms = outSyms[oi]; J.nRefs = outRefs[oi]; J.dcostTotal = dcPre[st.nChunks];
                J.outBase = splitSlots; J.maxBlocks = (int32_t)(outSyms[oi] / 8192 + 3); J.lastIsMatch = lastIsMatch;
                splitSlots += J.maxBlocks;
                preSym.insert(preSym.end(), symPre.begin(), symPre.end());
                preRef.insert(preRef.end(), refPre.begin(), refPre.end());
                preDc.insert(preDc.end(), dcPre.begin(), dcPre.end());
                splitJobs.push_back(J);
                splitOut.push_back(oi);
            }
        }
        std::vector<LzSplitOut> splitRes((size_t)splitSlots);
        std::vector<int32_t> splitCnt(splitJobs.size());
        if (!splitJobs.empty()) {
            RtScratch st;
            LzSplitJob* dJ = st.alloc<LzSplitJob>(splitJobs.size());
            long long *dA = st.alloc<long long>(preSym.size(), 16), *dBp = st.alloc<long long>(preSym.size(), 16), *dC = st.alloc<long long>(preSym.size(), 16);
            LzSplitOut* dO = st.alloc<LzSplitOut>((size_t)splitSlots, 16);
            int32_t* dCnt = st.alloc<int32_t>(splitJobs.size(), 16);
            rt_h2d(dJ, splitJobs.data(), splitJobs.size() * sizeof(LzSplitJob));
            rt_h2d(dA, preSym.data(), preSym.size() * 8);
            rt_h2d(dBp, preRef.data(), preRef.size() * 8);
            rt_h2d(dC, preDc.data(), preDc.size() * 8);
            RT_LAUNCH(k_lz_split, splitJobs.size(), 64, c, dJ, dA, dBp, dC, dO, dCnt);
            B.stats.kernel_launches++;
            rt_d2h(splitRes.data(), dO, (size_t)splitSlots * sizeof(LzSplitOut));
            rt_d2h(splitCnt.data(), dCnt, splitJobs.size() * 4);
            st.release();
        }
        size_t splitIdx = 0;
        for (size_t oi = 0; oi < nOut; oi++) {
            const LzSpecL& sp = specs[oi];
            const LzStream& st = hs[sp.input];
            LzOutStream& o = outs[oi];
            const i64 N = outSyms[oi], R = outRefs[oi];
            o.blkBase = (i64)blocks.size();
            auto push = [&](i64 symStart, i64 symCount, int isLast) {
                LzBlockDesc d;
                memset(&d, 0, sizeof(d));
                d.symStart = symStart; d.symCount = symCount; d.out = (int32_t)oi; d.isLast = isLast;
                d.uStart = d.uLen = st.len - st.dictLen; d.refStart = d.refCount = R;   // (an empty block: overwritten for the others)
                blocks.push_back(d);
            };
            if (sp.encoder == LZ_FLAVOR_JZLIB) {
                const LzSplitJob& J = splitJobs[splitIdx];
                int nb = splitCnt[splitIdx++];
                if (nb > J.maxBlocks) throw std::runtime_error("lz77: block list overflow");
                for (int b = 0; b < nb; b++) push(splitRes[J.outBase + b].symStart, splitRes[J.outBase + b].symCount, splitRes[J.outBase + b].isLast);
            } else {
                // zlib: a block is flushed after LZ_SYMS_PER_BLOCK symbols (lit_bufsize - 1).  The symbol that fills a
                // block exactly at the end of the input flushes it as a non-last block — and an empty last block
                // follows — unless it is the literal deflate_slow's epilogue emits after its loop (its flush flag is
                // ignored); deflate_huff, deflate_fast and deflate_rle have no such epilogue.
                const bool epilogueLiteral = kindOf[oi] == LZ_KIND_SLOW && !lastIsMatchOf[oi];
                i64 cur = 0;
                while (true) {
                    i64 take = std::min<i64>(LZ_SYMS_PER_BLOCK, N - cur);
                    bool endsStream = cur + take == N;
                    bool last = endsStream && (take < LZ_SYMS_PER_BLOCK || (N > 0 && epilogueLiteral));
                    push(cur, take, last);
                    cur += take;
                    if (last) break;
                    if (endsStream) { push(N, 0, 1); break; }
                }
            }
            o.nBlocks = (int32_t)(blocks.size() - o.blkBase);
            o.tokBase = tokTot;
            o.refBase = refTot;
            tokTot += N + o.nBlocks;
            refTot += R;
            for (int k = 0; k < std::max(1, (int)st.nChunks); k++)
                if (k == 0 || k >= first_chunk(sp.input))   // (chunk 0 also writes an empty last block's token; dictionary chunks hold none)
                    fillJobs.push_back({(int32_t)oi, (int32_t)k, k < st.nChunks ? symPreOf[oi][k] : 0, k < st.nChunks ? refPreOf[oi][k] : 0});
        }
        if (refTot >= (1LL << 32)) throw std::runtime_error("batch holds 2^32 or more back-references: split it");
        // ---- 4. tokens / records in the optimiser's layout ----
        RtEvent e3, e4;
        e3.record();
        B.dTok.alloc((size_t)tokTot, 64);
        B.dRefs.alloc((size_t)refTot, 64);
        B.dTokRef.alloc((size_t)tokTot, 64);
        const size_t nBlk = blocks.size();
        LzOutStream* dOuts = tmp.alloc<LzOutStream>(nOut, 16);
        LzBlockDesc* dBlk = tmp.alloc<LzBlockDesc>(nBlk, 16);
        LzFillJob* dFill = tmp.alloc<LzFillJob>(fillJobs.size(), 16);
        rt_h2d(dOuts, outs.data(), nOut * sizeof(LzOutStream));
        rt_h2d(dBlk, blocks.data(), nBlk * sizeof(LzBlockDesc));
        rt_h2d(dFill, fillJobs.data(), fillJobs.size() * sizeof(LzFillJob));
        if (!fillJobs.empty()) {
            RT_LAUNCH(k_lz_fill, fillJobs.size(), 64, c, dOuts, dFill, dBlk, B.dTok, B.dRefs, B.dTokRef);
            B.stats.kernel_launches++;
        }
        rt_d2h(blocks.data(), dBlk, nBlk * sizeof(LzBlockDesc));
        for (LzBlockDesc& d : blocks)
            if (d.symCount > 0) { d.uLen -= d.uStart; d.refCount -= d.refStart; }
            else { d.uLen = 0; d.refCount = 0; }
        rt_h2d(dBlk, blocks.data(), nBlk * sizeof(LzBlockDesc));
        // ---- 5. per block: zlib's trees and block type, and the block's state ----
        D4GState* dTmpStates = tmp.alloc<D4GState>(nBlk, 16);
        LzBlockOut* dBo = tmp.alloc<LzBlockOut>(nBlk, 16);
        std::vector<LzBlockOut> bo(nBlk);
        if (nBlk) {
            RT_LAUNCH(k_lz_blocks, nBlk, 64, dStreamsLz, dOuts, dBlk, (int)nBlk, B.dTok, dTmpStates, dBo);
            B.stats.kernel_launches++;
            rt_d2h(bo.data(), dBo, nBlk * sizeof(LzBlockOut));
        }
        e4.record();
        // ---- 6. the batch's own view: parsed-stream descriptions, layout, states in slot 0 ----
        B.ps.assign(nOut, Batch::PStream());
        for (size_t oi = 0; oi < nOut; oi++) {
            Batch::PStream& P = B.ps[oi];
            const LzOutStream& o = outs[oi];
            P.uBaseFixed = rawU[specs[oi].input];
            P.nU = rawLen[specs[oi].input];
            i64 spos = 0;
            for (int b = 0; b < o.nBlocks; b++) {
                const LzBlockDesc& d = blocks[o.blkBase + b];
                const LzBlockOut& r = bo[o.blkBase + b];
                Batch::PBlock pb;
                pb.type = r.type; pb.bfinal = d.isLast; pb.bitPos = 0; pb.endBit = 0;
                pb.nTok = d.symCount + 1; pb.uLen = d.uLen; pb.sizeBits = r.sizeBits; pb.nRef = d.refCount; pb.firstBatch = -1;
                pb.refSpan = d.refCount;
                    pb.hdrBits = r.hdrBits;
                P.blocks.push_back(pb);
                P.nTok += pb.nTok;
                spos += 3;
                if (r.type == D4G_STORED) {
                    i64 al = spos % 8;
                    al = al == 0 ? 0 : 8 - al;
                    spos += (d.uLen + 4) * 8 + al;
                } else spos += r.sizeBits;
            }
            P.sizeBits = spos;
            P.consumed = (spos + 7) / 8;
        }
        Batch::Layout LY;
        B.layout_blocks(merge, optimise, LY);
        if (nBlk) {
            std::vector<long long> dst(nBlk, -1);
            for (size_t oi = 0; oi < nOut; oi++)
                for (int b = 0; b < outs[oi].nBlocks; b++) {
                    const HBlock& hb = B.streams[oi].blocks[b];
                    if (hb.gpu >= 0) dst[outs[oi].blkBase + b] = B.hBlocks[hb.gpu].stateIdx;
                }
            RtScratch st;
            long long* dDst = st.alloc<long long>(nBlk, 16);
            rt_h2d(dDst, dst.data(), nBlk * 8);
            RT_LAUNCH(k_lz_place_states, nBlk, 256, dTmpStates, dDst, (int)nBlk, B.dStates);
            B.stats.kernel_launches++;
            rt_sync();
            st.release();
        }
        RtScratch bins;
        B.block_bins(LY.realBlocks, optimise, bins);
        rt_sync();
        bins.release();
        B.stats.ms_lz_sort = rt_elapsed_ms(e0, e1);
        B.stats.ms_lz_parse = rt_elapsed_ms(e1, e2);
        B.stats.ms_lz_emit = rt_elapsed_ms(e3, e4);
        B.stats.lz_symbols = 0;
        for (size_t oi = 0; oi < nOut; oi++) B.stats.lz_symbols += outSyms[oi];
        tmp.release();   // the sort arrays, chunk tokens and block tables are done with: the candidate search needs the memory
        B.check_device_errors();
        double t1 = now_ms();
        if (optimise) B.phase1();
        double t2 = now_ms();
        if (optimise && merge) B.phase_merge();
        double t3 = now_ms();
        B.phase_write();
        double t4 = now_ms();
        B.stats.ms_parse = t1 - t0;     // here: the encoder front end
        B.stats.ms_optimise = t2 - t1;
        B.stats.ms_merge = t3 - t2;
        B.stats.ms_write = t4 - t3;
        B.stats.ms_total = t4 - t0;
        B.stats.ms_search_kernels = B.msSearch;
        B.stats.search_bytes_algorithmic = B.stats.bytes_decoded + B.stats.bytes_out;
        B.release_scratch();
    }
};

// A batch as the drivers and the C ABI hold it: the Batch and, when its streams come from the encoder, the front end that
// fills it.  LzFront refers to its Batch, so the two are made in place and stay together.  The dictionary arguments (host
// memory, nDict = 0: none) have been checked by the caller, as for LzFront::create.
struct HostBatch {
    Batch impl;
    std::unique_ptr<LzFront> lz;   // set for encoder batches
    void create_encode(size_t n, const uint8_t* const* raw, const size_t* len, size_t nOut, const LzSpecL* spec, bool fromDevice = false, size_t nDict = 0,
                       const uint8_t* const* dict = nullptr, const size_t* dictLen = nullptr, const int32_t* dictOf = nullptr) {
        lz.reset(new LzFront(impl));
        lz->create(n, raw, len, nOut, spec, fromDevice, nDict, dict, dictLen, dictOf);
    }
    void create_encode(size_t n, const uint8_t* const* raw, const size_t* len, size_t nOut, const LzSpec* spec, bool fromDevice = false) {
        create_encode(n, raw, len, nOut, LzFront::at_level_9(n, nOut, spec).data(), fromDevice);   // (the level-9 entry points)
    }
};

}  // namespace d4g

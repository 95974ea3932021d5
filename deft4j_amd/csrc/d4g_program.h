// d4g_program.h — the candidate-search program generator and the per-process device objects every batch shares.
#pragma once
#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <vector>

#include "d4g_knobs.h"

namespace d4g {

typedef long long i64;

// ---------------------------------------------------------------------------------------
// Candidate-search program = DeflateStream.optimiseBlock (B/deflate/DeflateStream.java:343-490)
// unrolled into ops over state slots.  Op ids follow the reference's enumeration order, so
// "first strict minimum" is min over (size, op id, lane).
// ---------------------------------------------------------------------------------------
struct Program {
    std::vector<D4GOp> ops;
    std::vector<int> opLevel;
    std::vector<int> slotLevel;
    int nSlots = 1, nMasks = 1, nLevels = 0;
    std::vector<std::vector<int>> stateLevels, hdrLevels;
    RtBuf<D4GOp> dOps;
    RtBuf<int32_t> dLists;
    std::vector<std::pair<size_t, int>> stateOff, hdrOff;  // per level: (offset into dLists, count)
    int nRequested = 0;  // ops the plain unrolling would have emitted (for the record)
    std::set<int> hsCodes;  // distinct code-length sets among the header searches (for the record)

    // ---- symbolic identity of a state, used to emit every distinct computation once ----
    // A state is determined by (m, c, h): token mask, code lengths, header — each the result of a
    // symbolic function application of the ops below — plus g, the guard under which the reference
    // builds it at all (a null optimiseBlockNormal result or an unchanged recodedHuffmanFull removes
    // whole subtrees).  Two requests with the same key are the same computation on the same data, so
    // the later one can only repeat an earlier candidate of equal size and never wins the strict `<`.
    struct Sym { int m, c, h, g; };
    std::vector<Sym> sym;               // per slot
    std::map<std::vector<int>, int> ids;      // symbolic function application -> id
    std::map<std::vector<int>, int> slotOf;   // op key -> slot
    std::set<std::vector<int>> offered, searched;
    int nextId = 1;
    int id_of(std::vector<int> key) {
        auto it = ids.find(key);
        if (it != ids.end()) return it->second;
        return ids[key] = nextId++;
    }

    int new_slot(int level, Sym sy) { slotLevel.push_back(level); sym.push_back(sy); return nSlots++; }
    int emit_raw(int kind, int src, int dst, int arg, bool cand, bool needMask, int level) {
        D4GOp op;
        memset(&op, 0, sizeof(op));
        op.kind = kind;
        op.src = src;
        op.dst = dst;
        op.arg = arg;
        op.seq = cand ? (int)ops.size() : -1;
        op.maskSlot = needMask ? nMasks++ : -1;
        op.scratch = -1;
        op.scratchMask = -1;
        if (kind == OP_RECODE_FULL) {
            op.scratch = new_slot(level, sym[src]); new_slot(level, sym[src]);
            op.scratchMask = nMasks; nMasks += 2;
        }
        ops.push_back(op);
        opLevel.push_back(level);
        return (int)ops.size() - 1;
    }
    // offer `slot` as a candidate at this point of the enumeration unless an equal state was offered before
    void offer(int slot, int cond, int opIdx) {
        const Sym& y = sym[slot];
        std::vector<int> uncond = {y.m, y.c, y.h, y.g, 0}, withc = {y.m, y.c, y.h, y.g, cond};
        bool dup = offered.count(uncond) || offered.count(withc);
        if (dup) { if (opIdx >= 0) ops[opIdx].seq = -1; return; }
        offered.insert(withc);
        if (opIdx < 0) emit_raw(OP_CAND, slot, -1, 0, true, false, slotLevel[slot] + 1);
    }
    // generic state op: kind/arg applied to src; `cand` offers the result
    int state_op(int kind, int src, int arg, bool cand, bool needMask) {
        nRequested++;
        const Sym x = sym[src];
        Sym y = x;
        int cond = 0;
        switch (kind) {
        case OP_RECODE:
            if (arg & 1) y.m = id_of({OP_RECODE, x.m, x.c});
            y.c = id_of({-1, y.m});          // code rebuilt from the histogram of mask y.m
            y.h = id_of({-2, y.c});          // rewriteHeader(default flags) of those lengths
            break;
        case OP_OPT:
            y.m = id_of({OP_OPT, x.m, x.c});
            y.h = id_of({OP_OPT, x.h});
            if (arg & 1) { cond = id_of({-3, x.m, x.c, x.h}); y.g = id_of({-4, x.g, cond}); }
            break;
        case OP_LEAST:
            y.m = id_of({OP_LEAST, arg, x.m, x.c});
            break;
        case OP_POST: y.h = id_of({OP_POST, x.h}); break;
        case OP_PRUNEHDR: y.h = id_of({OP_PRUNEHDR, x.h}); break;
        case OP_RECODE_FULL:
            y.m = id_of({OP_RECODE_FULL, 0, x.m, x.c, x.h});
            y.c = id_of({OP_RECODE_FULL, 1, x.m, x.c, x.h});
            y.h = id_of({OP_RECODE_FULL, 2, x.m, x.c, x.h});
            cond = id_of({-5, x.m, x.c, x.h});
            y.g = id_of({-4, x.g, cond});
            break;
        case OP_TOFIXED_OPT:
            y.m = id_of({OP_TOFIXED_OPT, x.m});
            y.c = id_of({-6});
            y.h = 0;
            break;
        default: break;
        }
        std::vector<int> key = {kind, arg, x.m, x.c, x.h, x.g};
        auto it = slotOf.find(key);
        if (it != slotOf.end()) {
            if (cand) offer(it->second, cond, -1);
            return it->second;
        }
        int level = slotLevel[src] + 1;
        int dst = new_slot(level, y);
        int opIdx = emit_raw(kind, src, dst, arg, cand, needMask, level);
        slotOf[key] = dst;
        if (cand) offer(dst, cond, opIdx);
        return dst;
    }
    int OPT(int src, bool requireSaved, bool cand) { return state_op(OP_OPT, src, requireSaved ? 1 : 0, cand, true); }
    int RECODE(int src, bool prune, bool cand) { return state_op(OP_RECODE, src, prune ? 1 : 0, cand, prune); }
    int FULL(int src, bool cand) { return state_op(OP_RECODE_FULL, src, 0, cand, true); }
    int LEAST(int src, int mode) { return state_op(OP_LEAST, src, mode, false, true); }
    void HS(int base) {  // the 56 header candidates depend only on the base's token bits and code lengths
        nRequested++;
        const Sym& y = sym[base];
        std::vector<int> key = {y.m, y.c, y.g};
        if (!searched.insert(key).second) return;
        hsCodes.insert(y.c);
        emit_raw(OP_HDRSEARCH, base, -1, 0, true, false, slotLevel[base] + 1);
    }

    void aor(int t) {  // addOptimisedRecoded — DeflateStream.java:265-317
        int b1 = OPT(t, false, false);
        int b2 = OPT(RECODE(t, false, false), false, false);
        int pruned = RECODE(t, true, false);
        int b3 = OPT(pruned, false, false);
        int b4 = OPT(FULL(pruned, false), false, false);
        HS(b1);
        HS(b2);
        HS(b3);
        HS(b4);
    }
    void run(int x) {  // runOptimisationsCallback — :400-442
        int post = state_op(OP_POST, x, 0, true, false);
        OPT(post, true, true);
        aor(post);
        int prune = state_op(OP_PRUNEHDR, x, 0, true, false);
        OPT(prune, true, true);
        aor(prune);
        aor(LEAST(x, 0));
        aor(LEAST(x, 1));
    }
    void multi(int e) {  // runOptimisationsCallbackMulti — :443-463
        nRequested++;
        offer(e, 0, -1);
        run(e);
        int hr = RECODE(e, false, true);
        run(hr);
        int hp = RECODE(e, true, true);
        run(hp);
        int hpf = FULL(hp, true);
        run(hpf);
    }
    void build(bool fixedOrigin) {
        slotLevel.assign(1, 0);
        sym.assign(1, Sym{id_of({-10}), id_of({-11}), id_of({-12}), 0});
        int T = 0;
        // the current block itself is the incumbent: candidates equal to it can never be strictly smaller
        offered.insert({sym[0].m, sym[0].c, sym[0].h, 0, 0});
        int optimised = OPT(T, true, true);  // op 0: "optimised"; the stored candidate (host) ranks right after it
        int H, OH;
        if (fixedOrigin) {
            H = RECODE(T, false, false);
            OH = OPT(H, true, false);
        } else {
            H = T;
            OH = optimised;
        }
        multi(H);
        multi(OH);
        if (!fixedOrigin) state_op(OP_TOFIXED_OPT, H, 0, true, true);  // "default fixed-huffman"
        multi(LEAST(H, 0));
        multi(LEAST(H, 1));
        // drop ops whose result feeds no candidate and no header search (e.g. bases of a repeated search)
        {
            std::vector<int> producer(nSlots, -1);
            for (size_t i = 0; i < ops.size(); i++)
                if (ops[i].dst >= 0) producer[ops[i].dst] = (int)i;
            std::vector<char> live(ops.size(), 0);
            std::vector<int> stack;
            for (size_t i = 0; i < ops.size(); i++)
                if (ops[i].seq >= 0 || ops[i].kind == OP_HDRSEARCH || ops[i].kind == OP_CAND) { live[i] = 1; stack.push_back((int)i); }
            while (!stack.empty()) {
                int i = stack.back();
                stack.pop_back();
                int pr = producer[ops[i].src];
                if (pr >= 0 && !live[pr]) { live[pr] = 1; stack.push_back(pr); }
            }
            std::vector<D4GOp> kept;
            std::vector<int> keptLevel;
            for (size_t i = 0; i < ops.size(); i++)
                if (live[i]) {
                    D4GOp o = ops[i];
                    if (o.seq >= 0) o.seq = (int)kept.size();
                    kept.push_back(o);
                    keptLevel.push_back(opLevel[i]);
                }
            ops.swap(kept);
            opLevel.swap(keptLevel);
        }
        // optimise() results nothing builds on (they are offered / searched for headers only): the fused executor computes
        // their size without writing their tokens down (arg bit 8; the other executors read bit 0 only)
        {
            std::vector<int> stateUses(nSlots, 0);
            for (const D4GOp& o : ops)
                if (o.kind != OP_HDRSEARCH && o.kind != OP_CAND) stateUses[o.src]++;
            for (D4GOp& o : ops)
                if (o.kind == OP_OPT && stateUses[o.dst] == 0) o.arg |= 0x100;
        }
        nLevels = 0;
        for (int l : opLevel) nLevels = std::max(nLevels, l + 1);
        stateLevels.assign(nLevels, {});
        hdrLevels.assign(nLevels, {});
        for (size_t i = 0; i < ops.size(); i++)
            (ops[i].kind == OP_HDRSEARCH ? hdrLevels : stateLevels)[opLevel[i]].push_back((int)i);
        // Within a level the ops are independent; the long ones are dispatched first so that the short ones fill the
        // launch's tail (execution order only — candidate ranking goes by op id).
        auto cost = [&](int id) {
            switch (ops[id].kind) {
            case OP_RECODE_FULL: return 8;
            case OP_RECODE: return (ops[id].arg & 1) ? 6 : 4;
            case OP_OPT: case OP_TOFIXED_OPT: case OP_LEAST: return 2;
            default: return 1;
            }
        };
        for (auto& v : stateLevels) std::stable_sort(v.begin(), v.end(), [&](int x, int y) { return cost(x) > cost(y); });
    }
    void release() {
        dOps.reset(); dLists.reset();
        stateOff.clear(); hdrOff.clear();
    }
    void upload() {
        dOps.alloc(ops.size());
        rt_h2d(dOps, ops.data(), ops.size() * sizeof(D4GOp));
        std::vector<int32_t> lists;
        for (int l = 0; l < nLevels; l++) {
            stateOff.push_back({lists.size(), (int)stateLevels[l].size()});
            lists.insert(lists.end(), stateLevels[l].begin(), stateLevels[l].end());
            hdrOff.push_back({lists.size(), (int)hdrLevels[l].size()});
            lists.insert(lists.end(), hdrLevels[l].begin(), hdrLevels[l].end());
        }
        dLists.alloc(lists.size());
        rt_h2d(dLists, lists.data(), lists.size() * sizeof(int32_t));
        rt_sync();
    }
};

// The 56 (flags, prune) pairs in addOptimisedRecoded's loop order — DeflateStream.java:281-315
static void build_hdr_tables(uint8_t* flags, uint8_t* prune) {
    int k = 0;
    for (int noRepZeros = 0; noRepZeros < 2; noRepZeros++)
        for (int pr = 0; pr < 2; pr++)
            for (int noRep = 0; noRep < (noRepZeros ? 1 : 2); noRep++)
                for (int noZRep = (noRepZeros ? 1 : 0); noZRep < 2; noZRep++)
                    for (int noZRep2 = 0; noZRep2 < 2; noZRep2++)
                        for (int ohh = 1; ohh >= 0; ohh--) {
                            int base = (noRep ? F_NOREP : 0) | (noZRep ? F_NOZREP : 0) | (noZRep2 ? F_NOZREP2 : 0) | (noRepZeros ? F_NOREPZEROS : 0);
                            if (ohh) {
                                if (noRep) continue;
                                for (int use8 = 1; use8 >= 0; use8--)
                                    for (int use7 = 1; use7 >= 0; use7--) {
                                        if (!use8 && !use7) continue;
                                        flags[k] = (uint8_t)(base | F_OHH | (use8 ? F_USE8 : 0) | (use7 ? F_USE7 : 0));
                                        prune[k] = (uint8_t)pr;
                                        k++;
                                    }
                            } else {
                                flags[k] = (uint8_t)base;
                                prune[k] = (uint8_t)pr;
                                k++;
                            }
                        }
    if (k != 56) throw std::runtime_error("header flag table: expected 56 candidates");
}

struct Engine {  // per-process device objects shared by all batches
    Program progDyn, progFixed;
    RtBuf<uint8_t> dHdrTables;  // flags[64] + prune[64]
    RtBuf<long long> dOpStats;
    RtBuf<uint32_t> dCrcTab;   // [1024] slice-by-4 CRC-32 tables, then [32] x^(2^k) mod P
    int slotsPerBlock = 0, masksPerBlock = 0, maxOps = 0;
    bool ready = false, built = false;
    // d4g_shutdown: the device objects go back (a later d4g_init may pick another device)
    void release() {
        if (!ready) return;
        progDyn.release(); progFixed.release();
        dHdrTables.reset(); dOpStats.reset(); dCrcTab.reset();
        ready = false;
    }
    void init() {
        static std::mutex initMu;   // several host threads may arrive with the first batches
        std::lock_guard<std::mutex> lk(initMu);
        if (ready) return;
        if (!built) {
            progDyn.build(false);
            progFixed.build(true);
            built = true;
        }
        const int dbg = debug_program();
        if (dbg)
            fprintf(stderr, "program: %d ops requested, %zu emitted (%zu header searches over %zu distinct code-length sets), %d levels, %d slots, %d masks\n",
                    progDyn.nRequested, progDyn.ops.size(), (size_t)std::count_if(progDyn.ops.begin(), progDyn.ops.end(), [](const D4GOp& o) { return o.kind == OP_HDRSEARCH; }),
                    progDyn.hsCodes.size(), progDyn.nLevels, progDyn.nSlots, progDyn.nMasks);
        if (dbg >= 2)
            for (int l = 0; l < progDyn.nLevels; l++) {
                int kinds[16] = {0};
                for (int id : progDyn.stateLevels[l]) kinds[progDyn.ops[id].kind * 1 + 0]++;
                fprintf(stderr, "level %2d: OPT %d RECODE %d FULL %d LEAST %d POST %d PRUNEHDR %d TOFIXED %d CAND %d | hdr searches %zu\n", l, kinds[1], kinds[2],
                        kinds[3], kinds[4], kinds[5], kinds[6], kinds[7], kinds[8], progDyn.hdrLevels[l].size());
            }
        progDyn.upload();
        progFixed.upload();
        uint8_t tab[128];
        memset(tab, 0, sizeof(tab));
        build_hdr_tables(tab, tab + 64);
        dHdrTables.alloc(128);
        rt_h2d(dHdrTables, tab, 128);
        dOpStats.alloc_zero(D4F_NSTATS);
        {
            std::vector<uint32_t> t(1024 + 32);
            for (uint32_t i = 0; i < 256; i++) {
                uint32_t c = i;
                for (int k = 0; k < 8; k++) c = (c & 1) ? (c >> 1) ^ 0xedb88320u : c >> 1;
                t[i] = c;
            }
            for (int k = 1; k < 4; k++)
                for (uint32_t i = 0; i < 256; i++) t[k * 256 + i] = (t[(k - 1) * 256 + i] >> 8) ^ t[t[(k - 1) * 256 + i] & 0xff];
            auto mul = [](uint32_t a, uint32_t b) {
                uint32_t m = 1u << 31, p = 0;
                for (;;) {
                    if (a & m) { p ^= b; if ((a & (m - 1)) == 0) break; }
                    m >>= 1;
                    b = (b & 1) ? (b >> 1) ^ 0xedb88320u : b >> 1;
                }
                return p;
            };
            uint32_t p = 1u << 30;  // x^1
            t[1024] = p;
            for (int k = 1; k < 32; k++) t[1024 + k] = p = mul(p, p);
            dCrcTab.alloc(t.size());
            rt_h2d(dCrcTab, t.data(), t.size() * 4);
        }
        rt_sync();
        slotsPerBlock = std::max(progDyn.nSlots, progFixed.nSlots);
        masksPerBlock = std::max(progDyn.nMasks, progFixed.nMasks);
        // the fused executor carves its per-block tables out of the same pools (d4g_fused.h: d4f_glob, d4f_eset)
        slotsPerBlock = std::max<int>(slotsPerBlock, 2 + (int)((D4F_GLOB_BYTES + sizeof(D4GState) - 1) / sizeof(D4GState)));
        masksPerBlock = std::max<int>(masksPerBlock, D4F_MAXM + 2 * D4F_MAXC);
        maxOps = (int)std::max(progDyn.ops.size(), progFixed.ops.size());
        if ((i64)maxOps * 64 >= (1LL << D4G_KEY_SEQ_BITS)) throw std::runtime_error("program too long for the key layout");
        ready = true;
    }
};
inline Engine& engine() {   // one per context (d4g_rt.h): the programs live in that device's memory
    static Engine e[RT_MAX_CTX];
    return e[rt_ctx()];
}

}  // namespace d4g

// libdeft4g.hip — the single translation unit of libdeft4g.so (kernels + host + C ABI).
// Build: hipcc -O3 -std=c++17 --offload-arch=gfx950 -shared -fPIC -o libdeft4g.so libdeft4g.hip
// It holds the ABI's guard, its argument checks, its entry points and the debug hooks; the drivers are in the d4g_host*.h headers.
#include <mutex>

#include "d4g_host.h"
#include "d4g_host_recompress.h"
#include "d4g_host_find.h"

using namespace d4g;

struct d4g_batch : HostBatch {   // (lz: set for batches made by d4g_batch_create_encode*)
    int ctx = 0;   // the context (device) the batch lives on: every call with the batch works there
    std::unique_ptr<Recompressed> recomp;   // d4g_batch_run_recompress: absent until a recompression ran
    // d4g_batch_verify: verdict and first mismatch per stream, and the final stream's block list as the re-parse read it
    bool verified = false;
    std::vector<int32_t> verdict;
    std::vector<int64_t> firstMismatch;
    std::vector<std::vector<Batch::PBlock>> finalBlocks;
    bool grafted(size_t i) const { return recomp && recomp->grafted(i); }
    int64_t graft_saved(size_t i) const { return recomp ? recomp->saved[i] : 0; }   // bits
    // where stream i's final bytes live: the grafted recompression where it won
    DevBytes final_bytes(size_t i) const { return grafted(i) ? recomp->bytes(i) : impl.out_bytes(i); }
};

namespace {
// CompressionUtil calls in from a thread pool (C/CompressionUtil.java:111-117).  d4g_init / d4g_shutdown are exclusive;
// everything else runs concurrently: a batch belongs to the thread that is calling with it, every host thread has its own
// HIP streams (d4g_rt.h) and the shared pieces (memory pool, engine set-up) take their own locks.  The test-only CPU
// emulator is single-threaded, so its build keeps one library-wide lock.
std::mutex g_mu;
#ifdef D4G_HOSTSIM
#define D4G_API_LOCK() std::lock_guard<std::mutex> lk(g_mu)
#else
#define D4G_API_LOCK() do { } while (0)
#endif
thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
bool ready() { return rt().ready; }
// The context of the calling thread for this call: the batch's, or — for calls that create batches / one-shot calls — the
// thread's choice (d4g_set_device; context 0 unless it chose).
thread_local int g_tlsCtx = 0;
int g_nCtx = 0;   // contexts initialised (d4g_init: 1)
void enter_ctx(const d4g_batch* b) { rt_ctx() = b ? b->ctx : g_tlsCtx; }
bool rtp_ctx_ready(int k) {
#ifdef D4G_HOSTSIM
    return k < g_nCtx;
#else
    return rtp().ctx[k].ready;
#endif
}
// the calling thread works on context k for a scope (the _on creators); not ok: there is no such context
struct OnContext {
    const int keep = g_tlsCtx;
    const bool ok;
    explicit OnContext(int k) : ok(k >= 0 && k < RT_MAX_CTX && rtp_ctx_ready(k)) {
        if (ok) g_tlsCtx = k;
        else g_err = "no such context (d4g_init_devices)";
    }
    ~OnContext() { g_tlsCtx = keep; }
};

// Runs `body` (returns a D4G_* code); whatever it throws becomes D4G_ERR_RUNTIME with its text — nothing crosses extern "C".
template <class F>
int to_code(F&& body) {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return fail(D4G_ERR_RUNTIME, "out of host memory");
    } catch (const std::exception& ex) {
        return fail(D4G_ERR_RUNTIME, ex.what());
    } catch (...) {
        return fail(D4G_ERR_RUNTIME, "unknown exception");
    }
}
// The guard of every entry point that works on the device, taken once per call: the emulator's lock (before the context,
// which a second thread must not switch under the first), the batch's context or the thread's, the library initialised,
// the device bound, then `body` through to_code.  The GPU build takes no lock here.
template <class F>
int api(const d4g_batch* b, F&& body) {
    D4G_API_LOCK();
    enter_ctx(b);
    if (!ready()) return fail(D4G_ERR_NODEVICE, "d4g_init has not succeeded");
    return to_code([&] {
        bind_device();
        return body();
    });
}

// The caller's result arrays of a one-shot call.  They hold the defined "unchanged" values from the start (out[i] = NULL,
// out_len[i] = 0, status[i] = D4G_STREAM_UNCHANGED, the optional arrays cleared) and get them back, buffers freed, unless
// the call commits: a failed call hands back no buffers.
struct Outputs {
    size_t n;
    uint8_t** out;
    size_t* len;
    int32_t* status;
    int64_t* saved;
    int64_t* recompSaved;
    int32_t* winner;
    bool kept = false;
    Outputs(size_t n, uint8_t** out, size_t* len, int32_t* status = nullptr, int64_t* saved = nullptr, int64_t* recompSaved = nullptr,
            int32_t* winner = nullptr)
        : n(n), out(out), len(len), status(status), saved(saved), recompSaved(recompSaved), winner(winner) {
        reset();
    }
    ~Outputs() {
        if (kept) return;
        for (size_t i = 0; i < n; i++) free(out[i]);
        reset();
    }
    int commit(int rc) {
        kept = rc == D4G_OK;
        return rc;
    }
    void reset() {
        for (size_t i = 0; i < n; i++) {
            out[i] = nullptr;
            len[i] = 0;
            if (status) status[i] = D4G_STREAM_UNCHANGED;
            if (saved) saved[i] = 0;
            if (recompSaved) recompSaved[i] = 0;
            if (winner) winner[i] = -1;
        }
    }
};

// ---- the internal layer: what the public batch calls and the one-shot calls are made of (the guard held by the caller) ----
std::unique_ptr<d4g_batch> make_batch(size_t n, const uint8_t* const* in, const size_t* in_len) {
    std::unique_ptr<d4g_batch> b(new d4g_batch());
    b->ctx = rt_ctx();
    b->impl.create(n, in, in_len);
    return b;
}
// the dictionary arguments of the _dict entry points: empty when they are in order, else why not
std::string dict_refusal(size_t n, size_t n_dict, const uint8_t* const* dict, const size_t* dict_len, const int32_t* dict_of) {
    if (n_dict && (!dict || !dict_len)) return "null argument";
    for (size_t d = 0; d < n_dict; d++)
        if (!dict[d] && dict_len[d]) return "dictionary " + std::to_string(d) + " is NULL but has a length";
    for (size_t i = 0; dict_of && n_dict && i < n; i++)
        if (dict_of[i] < -1 || dict_of[i] >= (int64_t)n_dict) return "dict_of[" + std::to_string(i) + "] names no dictionary";
    return "";
}
// d4g_batch_create_dict: the arguments have passed dict_refusal
std::unique_ptr<d4g_batch> make_batch_dict(size_t n, const uint8_t* const* in, const size_t* in_len, size_t n_dict, const uint8_t* const* dict,
                                           const size_t* dict_len, const int32_t* dict_of) {
    std::unique_ptr<d4g_batch> b = make_batch(n, in, in_len);
    if (n_dict && dict_of) b->impl.set_dictionaries(n_dict, dict, dict_len, dict_of);
    return b;
}
static_assert(sizeof(LzSpec) == sizeof(d4g_encoder_spec), "spec layout");
static_assert(sizeof(LzSpecL) == sizeof(d4g_encoder_spec_level), "spec layout");
// every encoder batch of the ABI is made here, from specs with a level or (the level-9 entry points) without; dict...: n_dict, dict,
// dict_len, dict_of (host memory), which have passed dict_refusal
template <class Spec, class... Dict>
std::unique_ptr<d4g_batch> encode_batch(size_t n, const uint8_t* const* raw, const size_t* len, size_t nOut, const Spec* spec, Dict... dict) {
    std::unique_ptr<d4g_batch> e(new d4g_batch());
    e->ctx = rt_ctx();
    e->create_encode(n, raw, len, nOut, spec, false, dict...);
    return e;
}
// one stream, parsed (and decoded): d4g_size_bits_fallback, d4g_inflate
std::unique_ptr<d4g_batch> parse_one(const uint8_t* in, size_t len, bool decode, const uint8_t* dict = nullptr, size_t dict_len = 0) {
    const int32_t first = 0;
    std::unique_ptr<d4g_batch> b = make_batch_dict(1, &in, &len, dict_len ? 1 : 0, &dict, &dict_len, &first);
    b->impl.parse_only(decode);
    return b;
}
// a malloc'd copy of n bytes of device memory
uint8_t* host_copy(const void* src, size_t n) {
    uint8_t* p = (uint8_t*)malloc(n ? n : 1);
    if (!p) throw std::bad_alloc();
    rt_d2h(p, src, n);
    return p;
}
// a malloc'd copy of stream i's final bytes (the grafted recompression where it won)
uint8_t* final_copy(const d4g_batch& b, size_t i, size_t* len) {
    const DevBytes f = b.final_bytes(i);
    *len = f.len;
    return host_copy(f.p, f.len);
}
int32_t stream_status(const d4g_batch& b, size_t i) {
    const HStream& s = b.impl.streams[i];
    return s.status != 0 ? D4G_STREAM_PARSE_ERROR : ((s.saved > 0 || b.grafted(i)) ? D4G_STREAM_CHANGED : D4G_STREAM_UNCHANGED);
}
// ---- round-trip verification (verify_items, d4g_host.h) ----
const char* verdict_name(int v) {
    switch (v) {
        case VERIFY_OK: return "OK";
        case VERIFY_SKIPPED: return "SKIPPED";
        case VERIFY_PARSE: return "PARSE";
        case VERIFY_SIZE: return "SIZE";
        case VERIFY_LENGTH: return "LENGTH";
        default: return "BYTES";
    }
}
static_assert(VERIFY_OK == D4G_VERIFY_OK && VERIFY_SKIPPED == D4G_VERIFY_SKIPPED && VERIFY_PARSE == D4G_VERIFY_PARSE &&
              VERIFY_SIZE == D4G_VERIFY_SIZE && VERIFY_LENGTH == D4G_VERIFY_LENGTH && VERIFY_BYTES == D4G_VERIFY_BYTES, "verdict values");
// the first negative verdict as the call's failure
int verdicts_to_code(const std::vector<VerifyItem>& items, const std::vector<size_t>& index, const char* what) {
    for (size_t k = 0; k < items.size(); k++)
        if (items[k].verdict < 0)
            return fail(D4G_ERR_RUNTIME, std::string(what) + ": verification failed: stream " + std::to_string(index[k]) + " verdict " +
                                             std::to_string(items[k].verdict) + " (" + verdict_name(items[k].verdict) + ") first mismatch " +
                                             std::to_string((long long)items[k].first));
    return D4G_OK;
}
// ---- why a stream did not parse (Batch::diagnose, d4g_host.h) ----
static_assert(D4G_DIAG_OK == D4G_PARSE_OK && D4G_DIAG_EOF == D4G_PARSE_EOF && D4G_DIAG_BLOCK_TYPE == D4G_PARSE_BLOCK_TYPE &&
              D4G_DIAG_STORED_LENGTHS == D4G_PARSE_STORED_LENGTHS && D4G_DIAG_CODE_LENGTHS == D4G_PARSE_CODE_LENGTHS &&
              D4G_DIAG_LITLEN_SYMBOL == D4G_PARSE_LITLEN_SYMBOL && D4G_DIAG_DIST_SYMBOL == D4G_PARSE_DIST_SYMBOL &&
              D4G_DIAG_DISTANCE_TOO_FAR == D4G_PARSE_DISTANCE_TOO_FAR, "reason values");
const d4g_parse_error PARSE_ERROR_NONE = {D4G_PARSE_OK, -1, -1, -1, -1, -1};
// stream i of a parsed batch (the guard held by the caller; an encoder batch parses nothing: every stream is OK)
d4g_parse_error batch_parse_error(d4g_batch& b, size_t i) {
    if (b.lz || b.impl.ps[i].status == 0) return PARSE_ERROR_NONE;
    b.impl.diagnose();
    const Batch::ParseError& e = b.impl.parseErrors[i];
    return d4g_parse_error{e.reason, (int32_t)e.block, e.blockBit, e.bitPos, e.decoded, e.value};
}
// ---- what decodes before the first failure (Batch::recover, d4g_host_parse.h) ----
// where stream i's recovered bytes lie (device) and how many: a stream that parsed answers with its decoded bytes
const uint8_t* batch_recovered(d4g_batch& b, size_t i, size_t* len) {
    Batch& B = b.impl;
    if (b.lz || B.ps[i].status == 0) {
        *len = (size_t)B.streams[i].nU;
        return B.dU + B.streams[i].uBase;
    }
    B.recover();
    *len = (size_t)B.recLen[i];
    return *len ? B.dRecU + B.recBase[i] : nullptr;
}
// has the library written stream i's final bytes?  (an encoder batch writes every output; an optimiser batch only what changed)
bool stream_written(const d4g_batch& b, size_t i) {
    return b.lz ? b.impl.streams[i].status == 0 : stream_status(b, i) == D4G_STREAM_CHANGED;
}
// d4g_batch_verify: re-parse every written stream where it lies and compare its decoded bytes with the batch's own
int batch_verify(d4g_batch& b, const char* what, bool failOnNegative) {
    const size_t n = b.impl.streams.size();
    if (n && !b.impl.dOut) return fail(D4G_ERR_ARG, "the batch has not run");
    b.verdict.assign(n, VERIFY_SKIPPED);
    b.firstMismatch.assign(n, -1);
    b.finalBlocks.assign(n, {});
    std::vector<VerifyItem> items;
    std::vector<size_t> index;
    for (size_t i = 0; i < n; i++) {
        if (!stream_written(b, i)) continue;
        const HStream& s = b.impl.streams[i];
        VerifyItem it;
        it.bytes = b.final_bytes(i).p;
        it.len = b.final_bytes(i).len;
        it.want = b.impl.dU + s.uBase;
        it.wantLen = s.nU;
        it.dict = s.dict; it.dictLen = s.dictLen;   // the written stream is parsed against the dictionary the input was
        it.wantBits = s.sizeBitsIn - s.saved - b.graft_saved(i);   // what d4g_batch_stream_result lets the caller compute
        items.push_back(it);
        index.push_back(i);
    }
    VerifyTotals T;
    verify_items(items, false, T);
    for (size_t k = 0; k < items.size(); k++) {
        b.verdict[index[k]] = items[k].verdict;
        b.firstMismatch[index[k]] = items[k].first;
        b.finalBlocks[index[k]].swap(items[k].blocks);
    }
    b.verified = true;
    d4g_stats& st = b.impl.stats;
    st.ms_verify += T.ms; st.ms_verify_kernels += T.msKernels; st.verify_streams += T.streams; st.verify_bytes += T.bytes;
    return failOnNegative ? verdicts_to_code(items, index, what) : D4G_OK;
}
int verify_if_switched(d4g_batch& b, const char* what) { return verify_switch() ? batch_verify(b, what, true) : D4G_OK; }
// outputs that sit in device memory outside a batch (d4g_compress, d4g_zopfli_streams) against raw inputs already on the device
int verify_loose(std::vector<VerifyItem>& items, const char* what) {
    std::vector<size_t> index(items.size());
    for (size_t i = 0; i < index.size(); i++) index[i] = i;
    VerifyTotals T;
    verify_items(items, false, T);
    return verdicts_to_code(items, index, what);
}
// the one-shot results of a batch that ran: its stream j goes to slot idx[j] of the caller's arrays (slot j when idx is
// null); out[] only for changed streams
void results_into(const d4g_batch& b, const size_t* idx, uint8_t** out, size_t* out_len, int64_t* saved_bits, int32_t* status,
                  int64_t* recompress_saved) {
    for (size_t j = 0; j < b.impl.streams.size(); j++) {
        const size_t i = idx ? idx[j] : j;
        status[i] = stream_status(b, j);
        if (status[i] == D4G_STREAM_CHANGED) out[i] = final_copy(b, j, &out_len[i]);
        if (saved_bits) saved_bits[i] = b.impl.streams[j].status == 0 ? b.impl.streams[j].saved : 0;
        if (recompress_saved) recompress_saved[i] = b.graft_saved(j);
    }
}
// d4g_optimise_streams on the calling thread's context for the caller's streams idx[0..m) (0..m when idx is null)
void optimise_into(size_t m, const size_t* idx, const uint8_t* const* in, const size_t* in_len, bool merge, uint8_t** out,
                   size_t* out_len, int64_t* saved_bits, int32_t* status) {
    std::vector<const uint8_t*> p(m);
    std::vector<size_t> l(m);
    for (size_t j = 0; j < m; j++) { p[j] = in[idx ? idx[j] : j]; l[j] = in_len[idx ? idx[j] : j]; }
    std::unique_ptr<d4g_batch> b = make_batch(m, p.data(), l.data());
    b->impl.run(merge);
    if (verify_switch() && batch_verify(*b, "d4g_optimise_streams", true) != D4G_OK) throw std::runtime_error(g_err);
    results_into(*b, idx, out, out_len, saved_bits, status, nullptr);
}
// an encoder batch's outputs as the encoder emits them, to the caller's out[] (d4g_deflate_streams*)
int encode_into(d4g_batch& b, uint8_t** out, size_t* out_len) {
    b.lz->run(false, false);
    if (int rc = verify_if_switched(b, "d4g_deflate_streams")) return rc;
    for (size_t i = 0; i < b.impl.streams.size(); i++) {
        if (b.impl.streams[i].status != 0) return fail(D4G_ERR_ARG, "stream did not parse");
        out[i] = final_copy(b, i, &out_len[i]);
    }
    return D4G_OK;
}
// d4g_batch_create_encode_level and d4g_batch_create_encode_dict (n_dict = 0: the former), the guard held by the caller
int create_encode_into(d4g_batch** b, size_t n_in, const uint8_t* const* raw, const size_t* raw_len, size_t n_dict, const uint8_t* const* dict,
                       const size_t* dict_len, const int32_t* dict_of, size_t n_out, const d4g_encoder_spec_level* spec) {
    if ((n_in && (!raw || !raw_len)) || (n_out && !spec)) return fail(D4G_ERR_ARG, "null argument");
    const LzSpecL* sp = (const LzSpecL*)spec;
    for (size_t i = 0; i < n_out; i++) {
        const std::string why = lz_spec_refusal(sp[i], n_in);
        if (!why.empty()) return fail(D4G_ERR_ARG, why);
    }
    std::string why = dict_refusal(n_in, n_dict, dict, dict_len, dict_of);
    if (why.empty()) why = lz_dict_spec_refusal(n_out, sp, n_dict, dict_len, dict_of);
    if (!why.empty()) return fail(D4G_ERR_ARG, why);
    *b = encode_batch(n_in, raw, raw_len, n_out, sp, n_dict, dict, dict_len, dict_of).release();
    return D4G_OK;
}
// d4g_deflate_streams_level and d4g_deflate_streams_dict (n_dict = 0: the former): takes the guard
int deflate_streams_into(size_t n, const uint8_t* const* raw, const size_t* raw_len, int encoder, int level, int strategy, size_t n_dict,
                         const uint8_t* const* dict, const size_t* dict_len, const int32_t* dict_of, uint8_t** out, size_t* out_len) {
    if (n && (!raw || !raw_len || !out || !out_len)) return fail(D4G_ERR_ARG, "null argument");
    Outputs o(n, out, out_len);
    std::string why = lz_spec_refusal(LzSpecL{0, encoder, strategy, level}, 1);
    if (why.empty()) why = dict_refusal(n, n_dict, dict, dict_len, dict_of);
    if (!why.empty()) return fail(D4G_ERR_ARG, why);
    std::vector<LzSpecL> sp(n);
    for (size_t i = 0; i < n; i++) sp[i] = {(int32_t)i, encoder, strategy, level};
    why = lz_dict_spec_refusal(n, sp.data(), n_dict, dict_len, dict_of);
    if (!why.empty()) return fail(D4G_ERR_ARG, why);
    return o.commit(api(nullptr, [&] { return encode_into(*encode_batch(n, raw, raw_len, n, sp.data(), n_dict, dict, dict_len, dict_of), out, out_len); }));
}
// CMDUtil.optimise's per-stream loop on a batch made by d4g_batch_create (d4g_host_recompress.h)
int recompress_batch(d4g_batch& b, int mode, int iter, bool merge) {
    const std::string why = recompress_refusal(b.impl, mode);
    if (!why.empty()) return fail(D4G_ERR_ARG, why);
    b.recomp = recompress(b.impl, mode, iter, merge);
    return D4G_OK;
}

}  // namespace

extern "C" {

const char* d4g_last_error(void) { return g_err.c_str(); }

// one context: device + memory pool + programs (caller holds g_mu)
static int init_ctx(int ctx, int device_index) {
    rt_ctx() = ctx;
#ifndef D4G_HOSTSIM
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return fail(D4G_ERR_NODEVICE, "no HIP device available (libdeft4g has no CPU fallback)");
    if (device_index < 0 || device_index >= n) return fail(D4G_ERR_ARG, "device index out of range");
    if (rt().ready && rt().device != device_index)
        return fail(D4G_ERR_ARG, "already initialised on device " + std::to_string(rt().device) + ": call d4g_shutdown() before selecting another device");
    RT_CHECK(hipSetDevice(device_index));
    rt().device = device_index;
    pool_max_bytes(&rt_pool().maxHeldBytes);
#endif
    rt().ready = true;
    (void)rt();           // this thread's streams
    engine().init();
    return D4G_OK;
}

int d4g_init(int device_index) {
    std::lock_guard<std::mutex> lk(g_mu);
    const int rc = to_code([&] { return init_ctx(0, device_index); });
    if (rc == D4G_OK && g_nCtx < 1) g_nCtx = 1;
    rt_ctx() = g_tlsCtx;
    return rc;
}

int d4g_init_devices(int n, const int* device_index) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (n < 1 || n > RT_MAX_CTX || !device_index) return fail(D4G_ERR_ARG, "1 to 16 contexts");
    const int rc = to_code([&] {
        for (int k = 0; k < n; k++)
            if (int rck = init_ctx(k, device_index[k])) return rck;
        return D4G_OK;
    });
    if (rc == D4G_OK) g_nCtx = std::max(g_nCtx, n);
    rt_ctx() = g_tlsCtx;
    return rc;
}

int d4g_device_count(void) { return g_nCtx; }

int d4g_set_device(int context) {
    if (context < 0 || context >= RT_MAX_CTX || !rtp_ctx_ready(context)) return fail(D4G_ERR_ARG, "no such context (d4g_init_devices)");
    g_tlsCtx = context;
    rt_ctx() = context;
    return D4G_OK;
}

void d4g_shutdown(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    for (int k = 0; k < RT_MAX_CTX; k++) {
        rt_ctx() = k;
        if (!rt().ready) continue;
        to_code([&] {
            bind_device();
            rt_sync_all();
            engine().release();
#ifndef D4G_HOSTSIM
            rt_pool_release();
            {   // every host thread's streams of this context (no batch may be running: shutdown is exclusive by contract)
                std::vector<RtGlobals*> all;
                { std::lock_guard<std::mutex> lk2(rtp().mu); all = rtp().threads; }
                for (RtGlobals* g : all)
                    if (g->ctxIdx == k) g->destroy_streams();
            }
            rt().device = -1;
#endif
            return D4G_OK;
        });
        rt().ready = false;
    }
    g_nCtx = 0;
    g_tlsCtx = 0;
    rt_ctx() = 0;
}

d4g_batch* d4g_batch_create(size_t n, const uint8_t* const* in, const size_t* in_len) {
    d4g_batch* b = nullptr;
    api(nullptr, [&] {
        b = make_batch(n, in, in_len).release();
        return D4G_OK;
    });
    return b;
}

d4g_batch* d4g_batch_create_dict(size_t n, const uint8_t* const* in, const size_t* in_len, size_t n_dict, const uint8_t* const* dict,
                                 const size_t* dict_len, const int32_t* dict_of) {
    d4g_batch* b = nullptr;
    api(nullptr, [&] {
        const std::string why = dict_refusal(n, n_dict, dict, dict_len, dict_of);
        if (!why.empty()) return fail(D4G_ERR_ARG, why);
        b = make_batch_dict(n, in, in_len, n_dict, dict, dict_len, dict_of).release();
        return D4G_OK;
    });
    return b;
}

int d4g_batch_run(d4g_batch* b, int merge_blocks) {
    return api(b, [&] {
        if (!b) return fail(D4G_ERR_ARG, "null batch");
        if (b->lz) return fail(D4G_ERR_ARG, "encoder batch: use d4g_batch_run_encode");
        b->impl.run(merge_blocks != 0);
        return verify_if_switched(*b, "d4g_batch_run");
    });
}

d4g_batch* d4g_batch_create_encode(size_t n_in, const uint8_t* const* raw, const size_t* raw_len, size_t n_out,
                                   const d4g_encoder_spec* spec) {
    d4g_batch* b = nullptr;
    api(nullptr, [&] {
        if ((n_in && (!raw || !raw_len)) || (n_out && !spec)) return fail(D4G_ERR_ARG, "null argument");
        b = encode_batch(n_in, raw, raw_len, n_out, (const LzSpec*)spec).release();
        return D4G_OK;
    });
    return b;
}

int d4g_batch_run_encode(d4g_batch* b, int optimise, int merge_blocks) {
    return api(b, [&] {
        if (!b || !b->lz) return fail(D4G_ERR_ARG, "not an encoder batch");
        b->lz->run(optimise != 0, merge_blocks != 0);
        return verify_if_switched(*b, "d4g_batch_run_encode");
    });
}

d4g_batch* d4g_batch_create_encode_level(size_t n_in, const uint8_t* const* raw, const size_t* raw_len, size_t n_out,
                                         const d4g_encoder_spec_level* spec) {
    d4g_batch* b = nullptr;
    api(nullptr, [&] { return create_encode_into(&b, n_in, raw, raw_len, 0, nullptr, nullptr, nullptr, n_out, spec); });
    return b;
}

d4g_batch* d4g_batch_create_encode_dict(size_t n_in, const uint8_t* const* raw, const size_t* raw_len, size_t n_dict, const uint8_t* const* dict,
                                        const size_t* dict_len, const int32_t* dict_of, size_t n_out, const d4g_encoder_spec_level* spec) {
    d4g_batch* b = nullptr;
    api(nullptr, [&] { return create_encode_into(&b, n_in, raw, raw_len, n_dict, dict, dict_len, dict_of, n_out, spec); });
    return b;
}

int d4g_deflate_streams_level(size_t n, const uint8_t* const* raw, const size_t* raw_len, int encoder, int level, int strategy,
                              uint8_t** out, size_t* out_len) {
    return deflate_streams_into(n, raw, raw_len, encoder, level, strategy, 0, nullptr, nullptr, nullptr, out, out_len);
}

int d4g_deflate_streams_dict(size_t n, const uint8_t* const* raw, const size_t* raw_len, int encoder, int level, int strategy, size_t n_dict,
                             const uint8_t* const* dict, const size_t* dict_len, const int32_t* dict_of, uint8_t** out, size_t* out_len) {
    return deflate_streams_into(n, raw, raw_len, encoder, level, strategy, n_dict, dict, dict_len, dict_of, out, out_len);
}

int d4g_deflate_streams(size_t n, const uint8_t* const* raw, const size_t* raw_len, int encoder, int strategy, uint8_t** out,
                        size_t* out_len) {
    if (n && (!raw || !raw_len || !out || !out_len)) return fail(D4G_ERR_ARG, "null argument");
    Outputs o(n, out, out_len);
    return o.commit(api(nullptr, [&] {
        std::vector<LzSpec> sp(n);
        for (size_t i = 0; i < n; i++) sp[i] = {(int32_t)i, encoder, strategy};
        return encode_into(*encode_batch(n, raw, raw_len, n, sp.data()), out, out_len);
    }));
}

int d4g_batch_stream_result(d4g_batch* b, size_t i, int32_t* status, int64_t* saved_bits, size_t* out_len, size_t* consumed,
                            int64_t* size_bits_in) {
    if (!b || i >= b->impl.streams.size()) return fail(D4G_ERR_ARG, "bad stream index");
    const HStream& s = b->impl.streams[i];
    if (status) *status = stream_status(*b, i);
    if (saved_bits) *saved_bits = s.status == 0 ? s.saved : 0;
    if (out_len) *out_len = s.status == 0 ? b->final_bytes(i).len : 0;
    if (consumed) *consumed = (size_t)s.consumed;
    if (size_bits_in) *size_bits_in = s.status == 0 ? s.sizeBitsIn : -1;
    return D4G_OK;
}

int d4g_batch_copy_output(d4g_batch* b, size_t i, uint8_t* dst, size_t cap) {
    if (!b || i >= b->impl.streams.size()) return fail(D4G_ERR_ARG, "bad stream index");
    if (b->impl.streams[i].status != 0) return fail(D4G_ERR_ARG, "stream did not parse");
    const DevBytes f = b->final_bytes(i);
    if (cap < f.len) return fail(D4G_ERR_ARG, "output buffer too small");
    return api(b, [&] {
        rt_d2h(dst, f.p, f.len);
        return D4G_OK;
    });
}

int d4g_batch_copy_decoded(d4g_batch* b, size_t i, uint8_t* dst, size_t cap, size_t* len) {
    if (!b || i >= b->impl.streams.size()) return fail(D4G_ERR_ARG, "bad stream index");
    const HStream& s = b->impl.streams[i];
    if (s.status != 0) return fail(D4G_ERR_ARG, "stream did not parse");
    if (len) *len = (size_t)s.nU;
    if (!dst) return D4G_OK;
    if (cap < (size_t)s.nU) return fail(D4G_ERR_ARG, "output buffer too small");
    return api(b, [&] {
        rt_d2h(dst, b->impl.dU + s.uBase, (size_t)s.nU);
        return D4G_OK;
    });
}

int d4g_batch_parse(d4g_batch* b) {
    return api(b, [&] {
        if (!b) return fail(D4G_ERR_ARG, "null batch");
        if (b->impl.ran) return fail(D4G_ERR_ARG, "batch already ran");
        b->impl.ran = true;
        b->impl.parse_only(true);
        return D4G_OK;
    });
}

int d4g_batch_checksums(d4g_batch* b, size_t i, uint32_t* crc32, uint32_t* adler32, int64_t* isize) {
    if (!b || i >= b->impl.streams.size()) return fail(D4G_ERR_ARG, "bad stream index");
    if (b->impl.streams[i].status != 0) return fail(D4G_ERR_ARG, "stream did not parse");
    return api(b, [&] {
        b->impl.checksums();
        const D4GCsumOut& o = b->impl.csums[i];
        if (crc32) *crc32 = o.crc32;
        if (adler32) *adler32 = o.adler32;
        if (isize) *isize = o.isize;
        return D4G_OK;
    });
}

int d4g_batch_stats(d4g_batch* b, d4g_stats* st) {
    if (!b || !st) return fail(D4G_ERR_ARG, "null argument");
    *st = b->impl.stats;
    return D4G_OK;
}

void d4g_batch_destroy(d4g_batch* b) {   // deletes the batch whatever state the library is in (after d4g_shutdown too)
    D4G_API_LOCK();
    enter_ctx(b);
    try { bind_device(); } catch (...) {}
    delete b;
}

int d4g_optimise_streams(size_t n, const uint8_t* const* in, const size_t* in_len, int merge_blocks, uint8_t** out,
                         size_t* out_len, int64_t* saved_bits, int32_t* status) {
    if (n && (!in || !in_len || !out || !out_len || !status)) return fail(D4G_ERR_ARG, "null argument");
    Outputs o(n, out, out_len, status, saved_bits);
    return o.commit(api(nullptr, [&] {
        optimise_into(n, nullptr, in, in_len, merge_blocks != 0, out, out_len, saved_bits, status);
        return D4G_OK;
    }));
}

d4g_batch* d4g_batch_create_on(int context, size_t n, const uint8_t* const* in, const size_t* in_len) {
    OnContext on(context);
    return on.ok ? d4g_batch_create(n, in, in_len) : nullptr;
}

// DeflateFilesContainer.optimise(List<DeflateStream>, boolean) over every initialised context (K/DeflateFilesContainer.java:18-43:
// the streams are independent): longest-processing-time-first partition by compressed size, one host thread and one batch per
// context, no exchange between the devices; the outputs are gathered in the caller's arrays (host memory) in stream order.
// Each worker takes the guard on its own context; the calling thread takes none (in the emulator the workers queue on its lock).
int d4g_optimise_streams_sharded(size_t n, const uint8_t* const* in, const size_t* in_len, int merge_blocks, uint8_t** out,
                                 size_t* out_len, int64_t* saved_bits, int32_t* status) {
    const int nc = g_nCtx;
    if (nc <= 1) return d4g_optimise_streams(n, in, in_len, merge_blocks, out, out_len, saved_bits, status);
    if (n && (!in || !in_len || !out || !out_len || !status)) return fail(D4G_ERR_ARG, "null argument");
    Outputs o(n, out, out_len, status, saved_bits);
    return o.commit(to_code([&] {
        std::vector<size_t> order(n);
        for (size_t i = 0; i < n; i++) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return in_len[a] > in_len[b]; });
        std::vector<std::vector<size_t>> shard(nc);
        std::vector<unsigned long long> load(nc, 0);
        for (size_t i : order) {
            int r = 0;
            for (int k = 1; k < nc; k++) if (load[k] < load[r]) r = k;
            shard[r].push_back(i);
            load[r] += in_len[i];
        }
        std::vector<int> rcs(nc, D4G_OK);
        std::vector<std::string> errs(nc);
        Joiner workers;
        for (int k = 0; k < nc; k++) {
            std::sort(shard[k].begin(), shard[k].end());
            workers.threads.emplace_back([&, k]() {
                g_tlsCtx = k;   // this thread works on context k
                rcs[k] = api(nullptr, [&] {
                    optimise_into(shard[k].size(), shard[k].data(), in, in_len, merge_blocks != 0, out, out_len, saved_bits, status);
                    return D4G_OK;
                });
                if (rcs[k] != D4G_OK) errs[k].swap(g_err);
            });
        }
        workers.join();
        int rc = D4G_OK;
        for (int k = 0; k < nc; k++)
            if (rcs[k] != D4G_OK) { rc = rcs[k]; g_err.swap(errs[k]); }
        return rc;
    }));
}

d4g_batch* d4g_batch_create_dict_on(int context, size_t n, const uint8_t* const* in, const size_t* in_len, size_t n_dict,
                                    const uint8_t* const* dict, const size_t* dict_len, const int32_t* dict_of) {
    OnContext on(context);
    return on.ok ? d4g_batch_create_dict(n, in, in_len, n_dict, dict, dict_len, dict_of) : nullptr;
}

int d4g_size_bits_fallback(const uint8_t* in, size_t len, int64_t* bits) {
    if (!in || !bits) return fail(D4G_ERR_ARG, "null argument");
    return api(nullptr, [&] {
        std::unique_ptr<d4g_batch> b = parse_one(in, len, false);
        const Batch::PStream& o = b->impl.ps[0];
        *bits = o.status == 0 ? o.sizeBits : (int64_t)len * 8;  // B/Deft.java:48-54
        return D4G_OK;
    });
}

int d4g_inflate(const uint8_t* in, size_t len, uint8_t** out, size_t* out_len, size_t* consumed, int32_t* status) {
    return d4g_inflate_dict(in, len, nullptr, 0, out, out_len, consumed, status);
}

int d4g_inflate_dict(const uint8_t* in, size_t len, const uint8_t* dict, size_t dict_len, uint8_t** out, size_t* out_len, size_t* consumed,
                     int32_t* status) {
    if (!in || !out || !out_len || !status) return fail(D4G_ERR_ARG, "null argument");
    if (!dict && dict_len) return fail(D4G_ERR_ARG, "the dictionary is NULL but has a length");
    Outputs o(1, out, out_len);
    return o.commit(api(nullptr, [&] {
        std::unique_ptr<d4g_batch> b = parse_one(in, len, true, dict, dict_len);
        const Batch::PStream& p = b->impl.ps[0];
        if (consumed) *consumed = (size_t)p.consumed;
        *status = p.status != 0 ? D4G_STREAM_PARSE_ERROR : D4G_STREAM_UNCHANGED;
        if (p.status == 0) {
            *out = host_copy(b->impl.dU + b->impl.streams[0].uBase, (size_t)p.nU);
            *out_len = (size_t)p.nU;
        }
        return D4G_OK;
    }));
}

static_assert(D4G_FOUND_KIND_ZLIB == D4G_FOUND_ZLIB && D4G_FOUND_KIND_GZIP == D4G_FOUND_GZIP, "kind values");
int d4g_find_streams(size_t n, const uint8_t* const* file, const size_t* file_len, const d4g_find_options* opt, d4g_found_stream** found,
                     size_t* n_found, d4g_find_stats* stats) {
    return d4g_find_streams_dict(n, file, file_len, opt, 0, nullptr, nullptr, found, n_found, stats);
}

int d4g_find_streams_dict(size_t n, const uint8_t* const* file, const size_t* file_len, const d4g_find_options* opt, size_t n_dict,
                          const uint8_t* const* dict, const size_t* dict_len, d4g_found_stream** found, size_t* n_found, d4g_find_stats* stats) {
    if (!found || !n_found || (n && (!file || !file_len))) return fail(D4G_ERR_ARG, "null argument");
    const int known = (1 << D4G_FOUND_ZLIB) | (1 << D4G_FOUND_GZIP);
    if (opt && ((opt->kinds & ~known) || opt->min_decoded < 0)) return fail(D4G_ERR_ARG, "bad find options");
    if (n >= ((size_t)1 << 31)) return fail(D4G_ERR_ARG, "too many files");
    for (size_t i = 0; i < n; i++) {
        if (file_len[i] && !file[i]) return fail(D4G_ERR_ARG, "null argument");
        if (file_len[i] >= ((size_t)1 << 31)) return fail(D4G_ERR_ARG, "a file of 2 GiB or more");
    }
    if (n_dict >= 0x7fffff) return fail(D4G_ERR_ARG, "too many dictionaries");
    const std::string why = dict_refusal(0, n_dict, dict, dict_len, nullptr);
    if (!why.empty()) return fail(D4G_ERR_ARG, why);
    return api(nullptr, [&] {
        FindRun R;
        R.run(n, file, file_len, opt ? opt->kinds : 0, opt ? opt->min_decoded : 0, n_dict, dict, dict_len);
        d4g_found_stream* out = nullptr;
        if (!R.found.empty()) {
            out = (d4g_found_stream*)malloc(R.found.size() * sizeof(d4g_found_stream));
            if (!out) throw std::bad_alloc();
            memcpy(out, R.found.data(), R.found.size() * sizeof(d4g_found_stream));
        }
        *found = out;
        *n_found = R.found.size();
        if (stats) *stats = R.st;
        return D4G_OK;
    });
}

// ---- Zopfli encoder ----
int d4g_zopfli_streams(size_t n, const uint8_t* const* raw, const size_t* raw_len, int iterations, int splitting, int max_blocks,
                       size_t master_block, uint8_t** out, size_t* out_len) {
    if (n && (!raw || !raw_len || !out || !out_len)) return fail(D4G_ERR_ARG, "null argument");
    Outputs o(n, out, out_len);
    if (iterations < 1 || splitting < 0 || splitting > 2 || max_blocks < 0 || master_block > ((size_t)8 << 20)) return fail(D4G_ERR_ARG, "bad zopfli options");
    return o.commit(api(nullptr, [&] {
        ZfUpload up(n, raw, raw_len);
        ZfFront zf;
        zf.create(n, up.ptr.data(), up.len.data());
        std::vector<ZfSpec> specs;
        for (size_t i = 0; i < n; i++) {
            if (master_block == 0 && raw_len[i] > ((size_t)8 << 20)) return fail(D4G_ERR_ARG, "inputs above 8 MiB need a master block size");
            specs.push_back({(int32_t)i, iterations, splitting, max_blocks, (long long)master_block});
        }
        zf.encode(specs);
        if (debug_zopfli())
            fprintf(stderr, "[zopfli] inputs %zu: table %.1f ms, split %.1f ms, squeeze %.1f ms (%lld blocks, %lld position-iterations), final+emit %.1f ms\n", n,
                    zf.fig.msTable, zf.fig.msSplit, zf.fig.msSqueeze, (long long)zf.fig.blocks, (long long)zf.fig.positions, zf.fig.msEmit);
        if (verify_switch()) {
            std::vector<VerifyItem> items(n);
            for (size_t i = 0; i < n; i++) { items[i].bytes = zf.out_bytes(i).p; items[i].len = zf.out_bytes(i).len; items[i].want = up.ptr[i]; items[i].wantLen = (i64)raw_len[i]; }
            if (int rc = verify_loose(items, "d4g_zopfli_streams")) return rc;
        }
        for (size_t i = 0; i < n; i++) {
            out_len[i] = zf.out_bytes(i).len;
            out[i] = host_copy(zf.out_bytes(i).p, out_len[i]);
        }
        zf.release();
        return D4G_OK;
    }));
}

int d4g_debug_zopfli_table(const uint8_t* raw, size_t n, size_t end, uint16_t* len16, uint16_t* dist16, uint16_t* sublen) {
    if (!raw || !len16 || !dist16) return fail(D4G_ERR_ARG, "null argument");
    return api(nullptr, [&] {
        const uint8_t* rp[1] = {raw};
        size_t rl[1] = {n};
        ZfUpload up(1, rp, rl);
        ZfFront zf;
        zf.create(1, up.ptr.data(), up.len.data());
        if (end == 0 || end > n) end = n;
        if (end == 0) { zf.release(); return D4G_OK; }   // the empty input: no position, and no tail to look up
        zf.ensure_tails({{0, (i64)end}});
        const ZfFront::Tail& t = zf.tails.at({0, (i64)end});
        std::vector<uint32_t> table(n * 8 + 8), best(n + 8), pool(zf.pool.cap);
        rt_d2h(table.data(), zf.hIn[0].table, n * 32);
        rt_d2h(best.data(), zf.hIn[0].best, n * 4);
        rt_d2h(pool.data(), zf.pool.words, (size_t)zf.pool.cap * 4);
        if ((i64)end > t.start && t.table != zf.hIn[0].table + t.start * 8) {
            rt_d2h(table.data() + t.start * 8, t.table, (size_t)(end - t.start) * 32);
            rt_d2h(best.data() + t.start, t.best, (size_t)(end - t.start) * 4);
        }
        for (size_t i = 0; i < end; i++) {
            len16[i] = (uint16_t)(best[i] >> 16);
            dist16[i] = (uint16_t)(best[i] & 0xffff);
            if (!sublen) continue;
            int from = 3;
            auto fill = [&](uint32_t w) { for (int l = from; l <= (int)(w >> 16); l++) sublen[i * 259 + l] = (uint16_t)(w & 0xffff); from = (int)(w >> 16) + 1; };
            for (int c = 0; c < 8; c++) {
                const uint32_t w = table[i * 8 + c];
                if (!w) break;
                if (c == 7 && (w & ZF_POOL_LINK)) { for (const uint32_t* q = &pool[w & 0x7fffffffu]; *q; q++) fill(*q); break; }
                fill(w);
            }
        }
        zf.release();
        return D4G_OK;
    });
}

__global__ void __launch_bounds__(64) k_zf_debug_code_lengths(const uint32_t* freq, int n, int maxbits, uint32_t* out) {
    __shared__ ZfEvalLds E;
    const int lane = threadIdx.x & 63;
    for (int i = lane; i < ZF_NUM_LL; i += 64) { E.llc[i] = i < n ? freq[i] : 0; E.ll[i] = 0; }
    d4g_wave_sync();
    const int m = zf_sort_leaves(E.llc, n, E.u.pm.big[0].w, E.u.pm.big[0].sym, E.u.pm.big[0].list[1]);
    d4g_wave_sync();
    {   // the wave-wide builder (what the GPU's block-size evaluation uses for the lit/len and distance trees)
        ZfPmRef r = {E.u.pm.big[0].w, E.u.pm.big[0].sym, E.u.pm.big[0].list[0], E.u.pm.big[0].list[1], &E.u.pm.big[0].bits[0][0], 18, m, E.lvl[0]};
        zf_pm_wave(r, maxbits, E.ll);
    }
    d4g_wave_sync();
    for (int i = lane; i < n; i += 64) out[i] = E.ll[i];
}

int d4g_debug_zopfli_code_lengths(const uint32_t* freq, int n, int maxbits, uint32_t* lengths) {
    if (!freq || !lengths || n < 1 || n > ZF_NUM_LL || maxbits < 1 || maxbits > 15) return fail(D4G_ERR_ARG, "bad argument");
    return api(nullptr, [&] {
        RtScratch tmp;
        uint32_t* dF = tmp.alloc<uint32_t>(n);
        uint32_t* dO = tmp.alloc<uint32_t>(n);
        rt_h2d(dF, freq, n * 4);
        RT_LAUNCH(k_zf_debug_code_lengths, 1, 64, dF, n, maxbits, dO);
        rt_d2h(lengths, dO, n * 4);
        tmp.release();
        return D4G_OK;
    });
}

__global__ void __launch_bounds__(64) k_debug_cl_tree(const uint32_t* freq, int n, uint32_t* out, int32_t* limited) {
    __shared__ D4GHdrLds H;
    const int lane = threadIdx.x & 63;
    const long long h = (long long)blockIdx.x * 64 + lane;
    const bool live = h < n;
    uint32_t f[19];
#pragma unroll
    for (int s = 0; s < 19; s++) f[s] = live ? freq[h * 19 + s] : 0u;
    D4GClLens len;
    const bool deep = d4g_cl_lengths(&H, lane, [&](int s) { return f[s]; }, len);
    if (live) {
#pragma unroll
        for (int s = 0; s < 19; s++) out[h * 19 + s] = (uint32_t)len.get(s);
        limited[h] = deep ? 1 : 0;
    }
}

int d4g_debug_cl_tree_lengths(const uint32_t* freq, int n, uint32_t* lengths, int32_t* limited) {
    if (!freq || !lengths || !limited || n < 1) return fail(D4G_ERR_ARG, "bad argument");
    return api(nullptr, [&] {
        RtScratch tmp;
        uint32_t* dF = tmp.alloc<uint32_t>((size_t)n * 19);
        uint32_t* dO = tmp.alloc<uint32_t>((size_t)n * 19);
        int32_t* dL = tmp.alloc<int32_t>((size_t)n);
        rt_h2d(dF, freq, (size_t)n * 19 * 4);
        RT_LAUNCH(k_debug_cl_tree, (n + 63) / 64, 64, dF, n, dO, dL);
        rt_d2h(lengths, dO, (size_t)n * 19 * 4);
        rt_d2h(limited, dL, (size_t)n * 4);
        tmp.release();
        return D4G_OK;
    });
}

// rewriteHeader(flags) of one set of code lengths by one wave (d4g_wave_pack_header with the fused executor's tree step)
__global__ void __launch_bounds__(64) k_debug_pack_header(const uint8_t* lens320, int nLit, int nDist, int flags, uint16_t* pairs, uint8_t* clLen19,
                                                          int32_t* out4) {
    __shared__ __attribute__((aligned(16))) uint8_t lens[D4G_NLIT + D4G_NDIST];
    __shared__ uint16_t prs[D4G_MAXPAIRS];   // (a pair stands for at least one of the at most 320 lengths)
    __shared__ uint32_t clFreq[20];
    __shared__ uint8_t clLen[32];
    __shared__ __attribute__((aligned(16))) unsigned char tree[D4GClTree::bytes(1)];
    const int lane = threadIdx.x & 63;
    for (int i = lane; i < D4G_NLIT + D4G_NDIST; i += 64) lens[i] = lens320[i];
    __syncthreads();
    int nPairs, nCl, bits;
    d4g_wave_clear_cl_freq(clFreq);
    const int err = d4g_wave_pack_header(nLit + nDist, [&](int i) { return i < nLit ? (int)lens[i] : (int)lens[D4G_NLIT + i - nLit]; }, flags, prs, clFreq, clLen,
                                         [&](const uint32_t* f, uint8_t* l) { return d4g_wave_cl_tree<D4GFusedTrees>(tree, f, l); }, nPairs, nCl, bits);
    __syncthreads();
    for (int i = lane; i < nPairs; i += 64) pairs[i] = prs[i];
    if (lane < 19) clLen19[lane] = clLen[lane];
    if (lane == 0) { out4[0] = nPairs; out4[1] = nCl; out4[2] = bits; out4[3] = err; }
}

int d4g_debug_pack_header(const uint8_t* lens320, int nLit, int nDist, int flags, uint16_t* pairs, int32_t* nPairs, uint8_t* clLen19, int32_t* nCl,
                          int32_t* bits) {
    if (!lens320 || !pairs || !nPairs || !clLen19 || !nCl || !bits || nLit < 1 || nLit > D4G_NLIT || nDist < 1 || nDist > D4G_NDIST || flags < 0 ||
        flags > 255)
        return fail(D4G_ERR_ARG, "bad argument");
    return api(nullptr, [&] {
        RtScratch tmp;
        uint8_t* dL = tmp.alloc<uint8_t>(D4G_NLIT + D4G_NDIST);
        uint16_t* dP = tmp.alloc<uint16_t>(D4G_MAXPAIRS);
        uint8_t* dC = tmp.alloc<uint8_t>(19);
        int32_t* dO = tmp.alloc<int32_t>(4);
        rt_h2d(dL, lens320, D4G_NLIT + D4G_NDIST);
        RT_LAUNCH(k_debug_pack_header, 1, 64, dL, nLit, nDist, flags, dP, dC, dO);
        int32_t o[4];
        rt_d2h(o, dO, sizeof(o));
        rt_d2h(pairs, dP, (size_t)o[0] * 2);
        rt_d2h(clLen19, dC, 19);
        tmp.release();
        *nPairs = o[0]; *nCl = o[1]; *bits = o[2];
        return o[3] ? fail(D4G_ERR_RUNTIME, "the code-length tree could not be built") : D4G_OK;
    });
}

void d4g_free(void* p) { free(p); }

// ---- recompression (d4g_host_recompress.h) ----
int d4g_compress(size_t n, const uint8_t* const* raw, const size_t* raw_len, int mode, int iter, int merge_blocks, uint8_t** out,
                 size_t* out_len, int32_t* winner) {
    if (n && (!raw || !raw_len || !out || !out_len)) return fail(D4G_ERR_ARG, "null argument");
    Outputs o(n, out, out_len, nullptr, nullptr, nullptr, winner);
    return o.commit(api(nullptr, [&] {
        const std::string why = mode_refusal(mode);
        if (!why.empty()) return fail(D4G_ERR_ARG, why);
        CompressRun R;
        compress_run(R, n, raw, raw_len, false, mode, iter, merge_blocks != 0);
        if (verify_switch()) {
            ZfUpload up(n, raw, raw_len);
            std::vector<VerifyItem> items(n);
            for (size_t i = 0; i < n; i++) { items[i].bytes = R.win.p[i]; items[i].len = R.win.len[i]; items[i].want = up.ptr[i]; items[i].wantLen = (i64)raw_len[i]; }
            if (int rc = verify_loose(items, "d4g_compress")) return rc;
        }
        for (size_t i = 0; i < n; i++) {
            out[i] = host_copy(R.win.p[i], R.win.len[i]);
            out_len[i] = R.win.len[i];
            if (winner) winner[i] = (int32_t)R.winner[i];
        }
        return D4G_OK;
    }));
}

int d4g_batch_run_recompress(d4g_batch* b, int mode, int iter, int merge_blocks) {
    return api(b, [&] {
        if (!b || b->lz) return fail(D4G_ERR_ARG, "not a batch of deflate streams");
        if (int rc = recompress_batch(*b, mode, iter, merge_blocks != 0)) return rc;
        return verify_if_switched(*b, "d4g_batch_run_recompress");
    });
}

int d4g_batch_recompress_result(d4g_batch* b, size_t i, int32_t* grafted, int64_t* recompress_saved) {
    if (!b || i >= b->impl.streams.size()) return fail(D4G_ERR_ARG, "bad stream index");
    if (grafted) *grafted = b->grafted(i);
    if (recompress_saved) *recompress_saved = b->graft_saved(i);
    return D4G_OK;
}

int d4g_recompress_streams(size_t n, const uint8_t* const* in, const size_t* in_len, int mode, int iter, int merge_blocks,
                           uint8_t** out, size_t* out_len, int64_t* saved_bits, int64_t* recompress_saved, int32_t* status) {
    if (n && (!in || !in_len || !out || !out_len || !status)) return fail(D4G_ERR_ARG, "null argument");
    Outputs o(n, out, out_len, status, saved_bits, recompress_saved);
    return o.commit(api(nullptr, [&] {
        std::unique_ptr<d4g_batch> b = make_batch(n, in, in_len);
        if (int rc = recompress_batch(*b, mode, iter, merge_blocks != 0)) return rc;
        if (int rc = verify_if_switched(*b, "d4g_recompress_streams")) return rc;
        results_into(*b, nullptr, out, out_len, saved_bits, status, recompress_saved);
        return D4G_OK;
    }));
}

// ---- round-trip verification and per-block info ----
int d4g_batch_verify(d4g_batch* b) {
    return api(b, [&] {
        if (!b) return fail(D4G_ERR_ARG, "null batch");
        return batch_verify(*b, "d4g_batch_verify", false);
    });
}

int d4g_batch_verify_result(d4g_batch* b, size_t i, int32_t* verdict, int64_t* first_mismatch) {
    if (!b || i >= b->impl.streams.size()) return fail(D4G_ERR_ARG, "bad stream index");
    if (!b->verified) return fail(D4G_ERR_ARG, "the batch has not been verified (d4g_batch_verify)");
    if (verdict) *verdict = b->verdict[i];
    if (first_mismatch) *first_mismatch = b->firstMismatch[i];
    return D4G_OK;
}

int d4g_verify_streams(size_t n, const uint8_t* const* a, const size_t* a_len, const uint8_t* const* b, const size_t* b_len,
                       int32_t* verdict, int64_t* first_mismatch) {
    if (n && (!a || !a_len || !b || !b_len || !verdict)) return fail(D4G_ERR_ARG, "null argument");
    for (size_t i = 0; i < n; i++) { verdict[i] = D4G_VERIFY_SKIPPED; if (first_mismatch) first_mismatch[i] = -1; }
    return api(nullptr, [&] {
        std::unique_ptr<d4g_batch> A = make_batch(n, a, a_len);   // side a: parsed and decoded; its bytes stay in HBM
        A->impl.parse_only(true);
        std::vector<VerifyItem> items;
        std::vector<size_t> index;
        for (size_t i = 0; i < n; i++) {
            if (A->impl.ps[i].status != 0) continue;
            VerifyItem it;
            it.bytes = b[i]; it.len = b_len[i];
            it.want = A->impl.dU + A->impl.streams[i].uBase; it.wantLen = A->impl.streams[i].nU;
            items.push_back(it);
            index.push_back(i);
        }
        VerifyTotals T;
        verify_items(items, true, T);
        for (size_t k = 0; k < items.size(); k++) {
            verdict[index[k]] = items[k].verdict;
            if (first_mismatch) first_mismatch[index[k]] = items[k].first;
        }
        return D4G_OK;
    });
}

int d4g_batch_parse_error(d4g_batch* b, size_t i, d4g_parse_error* out) {
    return api(b, [&] {
        if (!b || !out) return fail(D4G_ERR_ARG, "null argument");
        if (i >= b->impl.streams.size()) return fail(D4G_ERR_ARG, "bad stream index");
        if (!b->lz && i >= b->impl.ps.size()) return fail(D4G_ERR_ARG, "the batch has not been parsed");
        *out = batch_parse_error(*b, i);
        return D4G_OK;
    });
}

int d4g_diagnose_streams(size_t n, const uint8_t* const* in, const size_t* in_len, d4g_parse_error* out) {
    if (n && (!in || !in_len || !out)) return fail(D4G_ERR_ARG, "null argument");
    for (size_t i = 0; i < n; i++) out[i] = PARSE_ERROR_NONE;
    return api(nullptr, [&] {
        std::unique_ptr<d4g_batch> b = make_batch(n, in, in_len);
        b->impl.parse_only(false);
        for (size_t i = 0; i < n; i++) out[i] = batch_parse_error(*b, i);
        return D4G_OK;
    });
}

int d4g_batch_recover(d4g_batch* b) {
    return api(b, [&] {
        if (!b) return fail(D4G_ERR_ARG, "null batch");
        if (b->lz) return D4G_OK;
        if (b->impl.ps.size() < b->impl.streams.size()) return fail(D4G_ERR_ARG, "the batch has not been parsed");
        b->impl.recover();
        return D4G_OK;
    });
}

int d4g_batch_copy_recovered(d4g_batch* b, size_t i, uint8_t* dst, size_t cap, size_t* len) {
    return api(b, [&] {
        if (!b) return fail(D4G_ERR_ARG, "null batch");
        if (i >= b->impl.streams.size()) return fail(D4G_ERR_ARG, "bad stream index");
        if (!b->lz && i >= b->impl.ps.size()) return fail(D4G_ERR_ARG, "the batch has not been parsed");
        if ((b->lz || b->impl.ps[i].status == 0) && b->impl.streams[i].nU > 0 && !b->impl.dU) return fail(D4G_ERR_ARG, "the batch has not been decoded");
        size_t n = 0;
        const uint8_t* src = batch_recovered(*b, i, &n);
        if (len) *len = n;
        if (!dst) return D4G_OK;
        if (cap < n) return fail(D4G_ERR_ARG, "output buffer too small");
        if (n) rt_d2h(dst, src, n);
        return D4G_OK;
    });
}

int d4g_recover_streams(size_t n, const uint8_t* const* in, const size_t* in_len, uint8_t** out, size_t* out_len, d4g_parse_error* why) {
    if (n && (!in || !in_len || !out || !out_len)) return fail(D4G_ERR_ARG, "null argument");
    for (size_t i = 0; why && i < n; i++) why[i] = PARSE_ERROR_NONE;
    Outputs o(n, out, out_len);
    const int rc = o.commit(api(nullptr, [&] {
        std::unique_ptr<d4g_batch> b = make_batch(n, in, in_len);
        b->impl.parse_only(true);
        for (size_t i = 0; i < n; i++) {
            const uint8_t* src = batch_recovered(*b, i, &out_len[i]);
            out[i] = host_copy(src, out_len[i]);
            if (why) why[i] = batch_parse_error(*b, i);
        }
        return D4G_OK;
    }));
    if (rc != D4G_OK)
        for (size_t i = 0; why && i < n; i++) why[i] = PARSE_ERROR_NONE;
    return rc;
}

const char* d4g_parse_reason_name(int reason) {   // (NULL, like the batch creators, when the guard refuses the call)
    static const char* const names[] = {"OK", "EOF", "BLOCK_TYPE", "STORED_LENGTHS", "CODE_LENGTHS", "LITLEN_SYMBOL", "DIST_SYMBOL", "DISTANCE_TOO_FAR"};
    const char* name = nullptr;
    api(nullptr, [&] {
        name = reason >= 0 && reason < (int)(sizeof(names) / sizeof(names[0])) ? names[reason] : "UNKNOWN";
        return D4G_OK;
    });
    return name;
}

int d4g_debug_batch_poke_output(d4g_batch* b, size_t i, size_t byte_offset, uint8_t xor_mask) {
    if (!b || i >= b->impl.streams.size()) return fail(D4G_ERR_ARG, "bad stream index");
    if (!b->impl.dOut || b->impl.streams[i].status != 0) return fail(D4G_ERR_ARG, "stream has no output");
    const DevBytes f = b->final_bytes(i);
    if (byte_offset >= f.len) return fail(D4G_ERR_ARG, "offset outside the stream's output");
    return api(b, [&] {
        uint8_t* at = (uint8_t*)f.p + byte_offset;
        uint8_t v = 0;
        rt_d2h(&v, at, 1);
        v ^= xor_mask;
        rt_h2d(at, &v, 1);
        rt_sync();
        return D4G_OK;
    });
}

int d4g_debug_batch_bins(d4g_batch* b, size_t block, uint32_t* table, uint64_t* masks, size_t mask_cap, uint32_t* records, size_t record_cap,
                         size_t* mask_words, size_t* n_records, size_t* n_blocks) {
    return api(b, [&] {
        if (!b) return fail(D4G_ERR_ARG, "null batch");
        if (b->lz) return fail(D4G_ERR_ARG, "an encoder batch");
        Batch& B = b->impl;
        if (!B.ran) B.run_parse(false);   // the parse of d4g_batch_run: d4g_batch_parse makes no tables
        if (n_blocks) *n_blocks = B.hBlocks.size();
        if (block >= B.hBlocks.size()) return fail(D4G_ERR_ARG, "bad block index");
        const D4GBlock& d = B.hBlocks[block];
        if (d.binStat < 0 || !B.dBinStat || !B.dBinMask || !B.dRefs) return fail(D4G_ERR_ARG, "the block has no table");
        const size_t mw = (size_t)d.maskWords, nr = (size_t)d.refCount;
        if (mask_words) *mask_words = mw;
        if (n_records) *n_records = nr;
        if ((masks && mask_cap < D4G_NBINS * mw) || (records && record_cap < nr)) return fail(D4G_ERR_ARG, "output buffer too small");
        if (table) rt_d2h(table, B.dBinStat + d.binStat, (size_t)D4G_NBINS * D4G_BINSTRIDE * 4);
        if (masks && mw) rt_d2h(masks, B.dBinMask + d.binMask, D4G_NBINS * mw * 8);
        if (records && nr) rt_d2h(records, B.dRefs + d.refStart, nr * 16);
        return D4G_OK;
    });
}

int d4g_debug_verify_compare(const uint8_t* x, size_t x_skew,const uint8_t* y, size_t y_skew, size_t len, int64_t* first) {
    if ((len && (!x || !y)) || !first || x_skew > 15 || y_skew > 15) return fail(D4G_ERR_ARG, "bad argument");
    return api(nullptr, [&] {
        RtScratch tmp;
        uint8_t* dX = tmp.alloc<uint8_t>(len, 64);
        uint8_t* dY = tmp.alloc<uint8_t>(len, 64);
        rt_h2d(dX + x_skew, x, len);
        rt_h2d(dY + y_skew, y, len);
        const D4GVerifyPair pr = {dX + x_skew, dY + y_skew, (long long)len};
        const long long base[2] = {0, ((long long)len + D4G_CSUM_TILE - 1) / D4G_CSUM_TILE};
        D4GVerifyPair* dPair = tmp.alloc<D4GVerifyPair>(1);
        long long* dBase = tmp.alloc<long long>(2);
        unsigned long long* dFirst = tmp.alloc<unsigned long long>(1);
        rt_h2d(dPair, &pr, sizeof(pr));
        rt_h2d(dBase, base, 16);
        rt_memset(dFirst, 0xff, 8);
        if (base[1]) RT_LAUNCH(k_verify_compare, base[1], 256, dPair, dBase, 1, dFirst);
        unsigned long long f = 0;
        rt_d2h(&f, dFirst, 8);
        tmp.release();
        *first = f == D4G_VERIFY_NONE ? -1 : (int64_t)f;
        return D4G_OK;
    });
}

int d4g_batch_block_info(d4g_batch* b, size_t i, int which, d4g_block_info* out, size_t cap, size_t* n_blocks) {
    if (!b || i >= b->impl.streams.size() || i >= b->impl.ps.size()) return fail(D4G_ERR_ARG, "bad stream index (or the batch has not been parsed)");
    if ((which != 0 && which != 1) || (cap && !out)) return fail(D4G_ERR_ARG, "bad argument");
    if (b->impl.ps[i].status != 0) return fail(D4G_ERR_ARG, "stream did not parse");
    const std::vector<Batch::PBlock>* list = &b->impl.ps[i].blocks;
    if (which == 1 && b->impl.dOut && stream_written(*b, i) && (b->lz == nullptr || b->impl.streams[i].saved > 0)) {
        // the final stream's blocks are read off the bytes that were written (the search's states are gone after a run)
        if (!b->verified)
            if (int rc = d4g_batch_verify(b)) return rc;
        if (b->finalBlocks[i].empty()) return fail(D4G_ERR_RUNTIME, "the final stream does not parse");
        list = &b->finalBlocks[i];
    }
    i64 pos = 0;   // DeflateStream.printBlockInfo (B/deflate/DeflateStream.java:35-51)
    for (size_t k = 0; k < list->size(); k++) {
        const Batch::PBlock& pb = (*list)[k];
        pos += 3;
        i64 size = pb.sizeBits;
        if (pb.type == D4G_STORED) {
            const i64 c = pos % 8;
            size = (pb.uLen + 4) * 8 + (c == 0 ? 0 : 8 - c);
        }
        if (k < cap) out[k] = d4g_block_info{pb.type, pb.bfinal, pos - 3, size + 3, pb.type == D4G_DYNAMIC ? pb.hdrBits : 0, pb.nTok, pb.uLen};
        pos += size;
    }
    if (n_blocks) *n_blocks = list->size();
    return D4G_OK;
}

#ifdef D4G_HOSTSIM
// emulator builds only: the closed-form pack summary against the reference-shaped loop, every flag set and run length
long long d4g_test_pack_kinds(void) {
    long long bad = 0;
    for (int flags = 0; flags < 256; flags++)
        for (int v = 0; v <= 7; v += 7)
            for (int r = 1; r <= 420; r++) {
                int a[19 * 160] = {0}, b[19 * 160] = {0};
                d4g_pack_run(v, r, flags, [&](int sym, int run, int) { a[sym * 160 + run]++; });
                d4g_pack_kinds(v, r, flags, [&](int sym, int run, int, int cnt) { b[sym * 160 + run] += cnt; }, [&](int cnt) { b[v * 160] += cnt; });
                for (int i = 0; i < 19 * 160; i++) bad += a[i] != b[i];
            }
    return bad;
}
#endif

// debug and tests only: device-memory blocks the calling thread's context has handed out and not yet got back
int d4g_debug_device_blocks(int64_t* live) {
    if (!live) return fail(D4G_ERR_ARG, "null argument");
    return api(nullptr, [&] {
        *live = (int64_t)rt_live_blocks();
        return D4G_OK;
    });
}

// dev tool: the fused executor's accounting (collected while D4G_FUSED_STATS is set; see k_search_fused); read and cleared
int d4g_debug_fused_stats(long long* out64) {
    return api(nullptr, [&] {
        engine().init();
        rt_sync_all();
        rt_d2h(out64, engine().dOpStats, 64 * 8);
        rt_memset(engine().dOpStats, 0, D4F_NSTATS * 8);
        rt_sync();
        return D4G_OK;
    });
}
// the same with the counters past the first 64 (the tree step's header accounting): out holds D4F_NSTATS (80) entries
int d4g_debug_fused_stats_all(long long* out80) {
    return api(nullptr, [&] {
        engine().init();
        rt_sync_all();
        rt_d2h(out80, engine().dOpStats, D4F_NSTATS * 8);
        rt_memset(engine().dOpStats, 0, D4F_NSTATS * 8);
        rt_sync();
        return D4G_OK;
    });
}

#ifdef D4G_PROFILE_OPS
// profiling builds only (scripts/build_profile_lib.sh): cycles and counts per op kind
int d4g_debug_set_experiment(long long mode) {
    return api(nullptr, [&] {
        rt_h2d(engine().dOpStats + 63, &mode, 8);
        rt_sync();
        return D4G_OK;
    });
}
int d4g_debug_opstats(long long* out64) {
    return api(nullptr, [&] {
        rt_d2h(out64, engine().dOpStats, 64 * 8);
        (void)hipMemcpyFromSymbol(out64 + 56, HIP_SYMBOL(d4g_dbg_counters), 7 * 8);
        (void)hipMemcpyFromSymbol(out64 + 16, HIP_SYMBOL(d4g_dbg_tree), 3 * 8);
        (void)hipMemcpyFromSymbol(out64 + 34, HIP_SYMBOL(d4g_dbg_pass), 4 * 8);
        return D4G_OK;
    });
}
#endif

}  // extern "C"

/* deft4g.h — C ABI of libdeft4g.so, the MI355X-native (gfx950, HIP) implementation of
 * deft4j's DEFLATE stream optimiser hot path.
 *
 * Every entry point replaces one seam of the Java reference (paths under /root/reference):
 *   B/ = deft4j-base/src/main/java/com/github/NeRdTheNed/deft4j/
 *   K/ = deft4j-container/src/main/java/com/github/NeRdTheNed/deft4j/container/
 *
 * Conventions: plain pointers and sizes only; inputs are borrowed for the duration of the
 * call; buffers returned through `uint8_t**` are allocated by the library and released with
 * d4g_free().  All functions return 0 on success and a negative value on failure (text in
 * d4g_last_error()).  Nothing here has a CPU fallback: without a usable HIP device
 * d4g_init() fails and every other call returns D4G_ERR_NODEVICE.
 *
 * SCOPE: mode NONE (parse, candidate search, mergeBlocks, write) and every recompress mode are built: the zlib-family
 * compressors (JavaCompressor / JZLibCompressor at level 9), the Zopfli compressors (CafeUndZopfli FIRST / LAST / NONE,
 * JZopfli's five option sets), CompressionUtil.compress and CMDUtil's recompress loop for modes CHEAP, ZOPFLI,
 * ZOPFLI_EXTENSIVE and ZOPFLI_VERY_EXTENSIVE.  An unknown mode returns D4G_ERR_ARG — never a substitute result.
 *
 * LIMITS (reported as errors of the call, never as a wrong result): one input of 2 GiB or more; 2^32 or more back-references
 * in one batch (split it); a Zopfli master block above 8 MiB (deft4j uses 8 MiB and 1 MB).
 *
 * THREADS: d4g_init / d4g_shutdown are exclusive.  Everything else may be called from several host threads at once
 * (CompressionUtil's pool, C/CompressionUtil.java:111-117): every thread gets its own HIP streams; a d4g_batch is used by
 * one thread at a time.
 */
#ifndef DEFT4G_H
#define DEFT4G_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D4G_OK 0
#define D4G_ERR_NODEVICE (-1)
#define D4G_ERR_ARG (-2)
#define D4G_ERR_RUNTIME (-3)

/* per-stream status, mirroring Deft.optimiseDeflateStream (B/Deft.java:21-34) */
#define D4G_STREAM_CHANGED 0     /* parse ok and bits saved > 0: use the new bytes            */
#define D4G_STREAM_UNCHANGED 1   /* parse ok, nothing saved: the caller keeps its ORIGINAL array */
#define D4G_STREAM_PARSE_ERROR (-1) /* DeflateStream.parse returned false: caller keeps the original */

typedef struct d4g_batch d4g_batch;

typedef struct d4g_stats {
    double ms_upload, ms_parse, ms_optimise, ms_merge, ms_write, ms_total; /* host wall clock per phase */
    int64_t n_streams, n_blocks, n_tokens, bytes_in, bytes_decoded, bytes_out;
    int64_t rounds, kernel_launches;
    int64_t search_bytes_algorithmic; /* C_in + U + C_out summed over streams */
    double ms_search_kernels;         /* device time of the candidate-search kernels (HIP events on the library's stream) */
    double ms_parse_kernels;          /* device time of scan + probe + emit + pointer-jumping kernels */
    int64_t scan_candidates, scan_confirmed, exact_probes, jump_rounds;
    double ms_state_kernels;          /* summed device time of k_exec_state_ops launches (HIP events around each launch) */
    int64_t state_launches;
    int64_t state_tokens_per_round, state_bytes_per_round; /* summed over k_exec_state_ops launches: tokens / decoded bytes of the blocks each launch covers */
    int64_t search_lanes;             /* block groups whose level sequences run concurrently (stream lanes) */
    double ms_checksum_kernels;       /* device time of the CRC-32 / Adler-32 kernels (d4g_batch_checksums) */
    /* encoder front end (d4g_batch_create_encode): device time of the hash sort, the lazy parse and the block emit */
    double ms_lz_sort, ms_lz_parse, ms_lz_emit;
    int64_t lz_parse_passes, lz_chunks_rerun, lz_symbols;
    /* d4g_batch_run_recompress: wall clock of the encode + optimise of every compressor output (front = encoder kernels,
     * search = candidate search on the encoder outputs) and of the re-parse + optimise of the winners */
    double ms_recompress_encode, ms_recompress_encode_front, ms_recompress_encode_search, ms_recompress_reoptimise;
    int64_t recompress_outputs;         /* compressor outputs that went through the candidate search */
    int64_t recompress_outputs_pruned;  /* HUFFMAN_ONLY outputs whose entropy bound already lost: not searched */
    /* Zopfli compressors (modes ZOPFLI*): wall clock of the match tables, the block-split searches, the squeeze kernel
     * and the block choice + emission; squeeze work = sum over blocks of iterations x block bytes */
    double ms_zopfli_table, ms_zopfli_split, ms_zopfli_squeeze, ms_zopfli_emit;
    int64_t zopfli_blocks, zopfli_position_iterations;
    /* fused executor (one workgroup per block, all rounds): optimiseBlock rounds it ran, rounds handed to the level executor */
    int64_t rounds_fused, fused_fallbacks;
    /* optimiseBlock rounds of long merged blocks run by the cluster kernel (the whole device on one block) */
    int64_t rounds_cluster;
    /* round-trip verification (d4g_batch_verify, D4G_VERIFY=1): wall clock; device time of the re-parse of the written
     * streams plus the byte compare (HIP events); streams verified; decoded bytes compared */
    double ms_verify, ms_verify_kernels;
    int64_t verify_streams, verify_bytes;
    /* decoded bytes by block-local copies (D4G_COPY, the default path): segments decoded (one workgroup each) and rounds of
     * the window scan; jump_rounds counts the rounds of the doubling path and stays 0 where no stream takes it */
    int64_t copy_segments, copy_rounds;
    /* recovery (d4g_batch_recover): failed streams whose leading bytes were decoded, those bytes, wall clock, and device time
     * of the count pass plus the side batch's emit and copy kernels */
    int64_t recover_streams, recover_bytes;
    double ms_recover, ms_recover_kernels;
    /* fused executor, which way a block left a launch: fused_fallbacks_mid = fallbacks (counted in fused_fallbacks too) of a
     * launch that had completed at least one round of that block; fused_relaunches = blocks launched again in k_search_fused,
     * after the per-launch round limit or after an improving level-executor round; cluster_fallbacks = rounds the cluster
     * kernel could not hold and handed to the level executor */
    int64_t fused_fallbacks_mid, fused_relaunches, cluster_fallbacks;
    /* header scan: scan_candidates = bit positions with a plausible prolog and a complete code-length code; scan_kept = those
     * whose coded code lengths also give complete codes, which is what the probe is run on */
    int64_t scan_kept;
    /* preset dictionaries (d4g_batch_create_dict): streams of the batch that have one (of non-zero length), and the bytes of
     * dictionary tails uploaded — each dictionary once, its last 32 768 bytes at most, however many streams name it (an
     * encoder batch, d4g_batch_create_encode_dict: once per input that names it, in front of the input) */
    int64_t dict_streams, dict_bytes;
} d4g_stats;

/* Select the HIP device (one process per GPU) and create the library's stream.
 * Fails (D4G_ERR_NODEVICE) when no device is usable. */
int d4g_init(int device_index);
void d4g_shutdown(void);
/* ---- several GPUs in one process (a JVM is one process; CompressionUtil's pool, C/CompressionUtil.java:99-117, and
 * DeflateFilesContainer.optimise's stream list, K/DeflateFilesContainer.java:18-43, are what fans out over them) ----
 * A *context* is one device with its own memory pool and programs; context k = device_index[k] (a device may back more than
 * one context).  d4g_init(d) == context 0 on device d.  A batch lives on the context it was created on and every call with it
 * works there, from any host thread; calls that create batches (d4g_batch_create, the one-shot calls) use the calling thread's
 * context: 0 unless the thread chose another with d4g_set_device. */
int d4g_init_devices(int n, const int* device_index);
int d4g_device_count(void);                 /* contexts initialised */
int d4g_set_device(int context);            /* the calling thread's context from now on */
const char* d4g_last_error(void);

/* ---- batch API: K/DeflateFilesContainer.java:18-43 `optimise(List<DeflateStream>, boolean)` ----
 * Streams are independent.  create() copies the inputs to HBM; run() does all device work
 * (parse -> optimise -> [mergeBlocks] -> write) with inputs and outputs resident in HBM. */
d4g_batch* d4g_batch_create(size_t n, const uint8_t* const* in, const size_t* in_len);
d4g_batch* d4g_batch_create_on(int context, size_t n, const uint8_t* const* in, const size_t* in_len);
/* ---- preset dictionaries: streams written with deflateSetDictionary / Deflater.setDictionary / zdict= ----
 * The rule is zlib's inflateSetDictionary on a raw stream.  Let L = min(dict_len, 32768): only the dictionary's last L bytes
 * count.  At decoded position p a distance d is valid iff d <= p + L, and the byte at q = p - d < 0 is dict_tail[L + q]; a
 * copy may begin in the dictionary and run on into the stream's own bytes, overlapping itself like any copy.  The dictionary
 * is not part of the decoded bytes: decoded_len, CRC-32, Adler-32, ISIZE, decoded_offset, d4g_block_info.decoded_len and
 * bytes_decoded do not count it.  A dictionary of length 0, or none, is d4g_batch_create exactly: the same kernels, the same
 * device blocks.
 * dict_of[i] = index of stream i's dictionary, -1: none; dict_of NULL or n_dict 0: d4g_batch_create.  Every dictionary's tail
 * is uploaded once per batch.  Refused (NULL, D4G_ERR_ARG in d4g_last_error's sense): a dict_of value outside -1..n_dict-1, a
 * NULL dictionary with a length.
 * Everything a batch can be asked works on such a batch — parse, run with and without mergeBlocks, outputs, decoded bytes,
 * checksums, block info, parse errors (DISTANCE_TOO_FAR by the rule above), recovery, and verification, which parses the
 * written stream again with the same dictionary — except d4g_batch_run_recompress with a mode above NONE: its jzlib and
 * Zopfli compressors take no dictionary, so a batch that holds any dictionary stream is refused there with D4G_ERR_ARG.  (The
 * zlib-flavour LZ77 encoder does write dictionary streams from raw data: d4g_batch_create_encode_dict, below.) */
d4g_batch* d4g_batch_create_dict(size_t n, const uint8_t* const* in, const size_t* in_len, size_t n_dict, const uint8_t* const* dict,
                                 const size_t* dict_len, const int32_t* dict_of);
d4g_batch* d4g_batch_create_dict_on(int context, size_t n, const uint8_t* const* in, const size_t* in_len, size_t n_dict,
                                    const uint8_t* const* dict, const size_t* dict_len, const int32_t* dict_of);
int d4g_batch_run(d4g_batch* b, int merge_blocks);
/* status: D4G_STREAM_*; saved_bits = DeflateStream.optimise(mergeBlocks) (B/deflate/DeflateStream.java:496);
 * out_len = bytes DeflateStream.asBytes() (:652) would return; consumed = input bytes parse() read
 * (byte-exact, K/GZFile.java:84 depends on it); size_bits_in = DeflateStream.getSizeBits() (:171) of the input. */
int d4g_batch_stream_result(d4g_batch* b, size_t i, int32_t* status, int64_t* saved_bits, size_t* out_len,
                            size_t* consumed, int64_t* size_bits_in);
/* copy stream i's re-serialised bytes (DeflateStream.write, :128-145) to host memory */
int d4g_batch_copy_output(d4g_batch* b, size_t i, uint8_t* dst, size_t cap);
/* copy stream i's decoded bytes (DeflateStream.getUncompressedData, :159-169) */
int d4g_batch_copy_decoded(d4g_batch* b, size_t i, uint8_t* dst, size_t cap, size_t* len);
/* Trailer values of stream i computed on the device from its decoded bytes: CRC-32 and ISIZE as
 * K/GZFile.java:129-145 recomputes them (java.util.zip.CRC32), Adler-32 as K/ZLibFile.java:41-51 does.
 * Valid after d4g_batch_run (or d4g_batch_parse). */
int d4g_batch_checksums(d4g_batch* b, size_t i, uint32_t* crc32, uint32_t* adler32, int64_t* isize);
/* parse + decode only (DeflateStream.parse for every stream); makes copy_decoded / checksums available */
int d4g_batch_parse(d4g_batch* b);
int d4g_batch_stats(d4g_batch* b, d4g_stats* st);
void d4g_batch_destroy(d4g_batch* b);

/* ---- encoder front end: the LZ77 compressors behind deft4j's recompress modes ----
 * One d4g_encoder_spec = one output of one Compressor object in CompressionUtil.getCompressors
 * (deft4j-compress/.../util/compression/CompressionUtil.java:44-78):
 *   D4G_ENC_JVM    JavaCompressor   (JavaCompressor.java:36-49): java.util.zip.Deflater(BEST_COMPRESSION, nowrap) = zlib level 9
 *   D4G_ENC_JZLIB  JZLibCompressor  (JZLibCompressor.java:29-41): jzlib 1.1.x level 9 (same algorithm, early block flush)
 * with strategy DEFAULT / FILTERED / HUFFMAN_ONLY.  The batch's streams are the specs' outputs, in order; several specs
 * may name the same input (its hash chains are built once).  run_encode(optimise = 0) leaves every stream exactly as the
 * encoder emits it (SingleCompressor.compressSingle); optimise = 1 also runs Deft.optimiseDeflateStream on it
 * (CompressorTask.java:29-35) without serialising and re-parsing the encoder's output.  Results come through
 * d4g_batch_stream_result / d4g_batch_copy_output: size_bits_in = bit size of the encoder's own output, saved_bits = what
 * the optimiser took off it. */
#define D4G_ENC_JVM 0
#define D4G_ENC_JZLIB 1
#define D4G_STRATEGY_DEFAULT 0
#define D4G_STRATEGY_FILTERED 1
#define D4G_STRATEGY_HUFFMAN_ONLY 2
typedef struct d4g_encoder_spec { int32_t input, encoder, strategy; } d4g_encoder_spec;
d4g_batch* d4g_batch_create_encode(size_t n_in, const uint8_t* const* raw, const size_t* raw_len, size_t n_out,
                                   const d4g_encoder_spec* spec);
int d4g_batch_run_encode(d4g_batch* b, int optimise, int merge_blocks);
/* SingleCompressor.compressSingle for n inputs with one encoder setting: out[i] is always set (release with d4g_free) */
int d4g_deflate_streams(size_t n, const uint8_t* const* raw, const size_t* raw_len, int encoder, int strategy, uint8_t** out,
                        size_t* out_len);
/* The same encoders at a compression level (java.util.zip.Deflater / zlib levels): output byte-identical to zlib 1.2.11
 * deflateInit2(level, Z_DEFLATED, -15, 8, strategy).  Levels 1-3 run deflate_fast, 4-9 deflate_slow with zlib's
 * configuration table; -1 (Z_DEFAULT_COMPRESSION) means 6.  Strategies add Z_RLE (distance-1 runs, any level) and
 * Z_FIXED (the level's parse, fixed trees or stored blocks only).  Refused with D4G_ERR_ARG / a NULL batch: level 0
 * (deflate_stored's blocks depend on the caller's output buffer), levels outside -1..9, and the jzlib flavour at any
 * level but 9 or with RLE / FIXED.  The result of d4g_batch_create_encode_level runs with d4g_batch_run_encode. */
#define D4G_STRATEGY_RLE 3
#define D4G_STRATEGY_FIXED 4
typedef struct d4g_encoder_spec_level { int32_t input, encoder, strategy, level; } d4g_encoder_spec_level;
d4g_batch* d4g_batch_create_encode_level(size_t n_in, const uint8_t* const* raw, const size_t* raw_len, size_t n_out,
                                         const d4g_encoder_spec_level* spec);
int d4g_deflate_streams_level(size_t n, const uint8_t* const* raw, const size_t* raw_len, int encoder, int level, int strategy,
                              uint8_t** out, size_t* out_len);
/* The same with preset dictionaries: output byte-identical to zlib 1.2.11 deflateInit2(level, Z_DEFLATED, -15, 8, strategy)
 * followed by deflateSetDictionary(dict, dict_len) — raw DEFLATE, no header: a zlib wrapper's DICTID is the Adler-32 of the
 * whole dictionary as passed.  zlib 1.2.11's rule: only the dictionary's last 32 768 bytes count, all of its strings are
 * inserted at every level, and the stream is what deflate would write from position L of tail || input on; a dictionary of
 * length 0 is none, and HUFFMAN_ONLY ignores it.  dict_of[i] = index of INPUT i's dictionary, -1: none; dict_of NULL or
 * n_dict 0: the calls above.  The dictionary arguments are checked as d4g_batch_create_dict checks them.  The batch's
 * streams carry their dictionary: run_encode with optimise = 1, verification (D4G_VERIFY, d4g_batch_verify), block info and
 * checksums work as on a d4g_batch_create_dict batch.
 * Scope limits: the jzlib flavour with a dictionary is refused (D4G_ERR_ARG / NULL) — jzlib's setDictionary follows the older
 * zlib rule (a 32 506-byte tail, the last two strings never inserted, dictionaries under 3 bytes ignored), which nothing
 * here can pin; the Zopfli encoder takes no dictionary; d4g_batch_run_recompress keeps refusing dictionary batches. */
d4g_batch* d4g_batch_create_encode_dict(size_t n_in, const uint8_t* const* raw, const size_t* raw_len, size_t n_dict,
                                        const uint8_t* const* dict, const size_t* dict_len, const int32_t* dict_of /* per input, -1 = none */,
                                        size_t n_out, const d4g_encoder_spec_level* spec);
int d4g_deflate_streams_dict(size_t n, const uint8_t* const* raw, const size_t* raw_len, int encoder, int level, int strategy,
                             size_t n_dict, const uint8_t* const* dict, const size_t* dict_len, const int32_t* dict_of, uint8_t** out,
                             size_t* out_len);

/* ---- recompress modes (deft4j-cmd/.../cmd/CMDUtil.java:44-50, Optimise.java `--mode`) ----
 * mode = ordinal of RecompressMode: the compressor list CompressionUtil.getCompressors builds for it (:44-78), in list
 * order JVM{DEFAULT, FILTERED, HUFFMAN_ONLY}, [JZopfli], [CafeUndZopfli], JZlib{DEFAULT, FILTERED, HUFFMAN_ONLY}.
 * `iter` = Zopfli iterations (-I of the reference CLI, default 20), used by the modes from ZOPFLI up. */
/* ---- Zopfli encoder (the recompress modes ZOPFLI / ZOPFLI_EXTENSIVE / ZOPFLI_VERY_EXTENSIVE) ----
 * MultiCafeUndZopfliCompressor.compressWithOptions (C/MultiCafeUndZopfliCompressor.java:48-52: CafeUndZopfli, master block
 * 8 << 20, BlockSplitting FIRST / LAST / NONE, `iter` iterations) and MultiJZopfliCompressor.compressWithOptions
 * (C/MultiJZopfliCompressor.java:78-85: jzopfli, master block 1000000, blocksplittingmax 15 or 0) for n inputs with one
 * option set: out[i] is a complete raw deflate stream (release with d4g_free).  splitting: D4G_ZOPFLI_SPLIT_*;
 * max_blocks: 0 = unlimited; master_block: bytes per independently encoded part (0 = the whole input; at most 8 MiB).
 * The dependencies themselves are not in the reference tree: the algorithm is the published Zopfli, pinned through
 * oracle/zopfli_oracle.c to libzopfli 1.0.3 and the reference's own asyoulik-zopfli fixture. */
#define D4G_ZOPFLI_SPLIT_FIRST 0
#define D4G_ZOPFLI_SPLIT_LAST 1
#define D4G_ZOPFLI_SPLIT_NONE 2
int d4g_zopfli_streams(size_t n, const uint8_t* const* raw, const size_t* raw_len, int iterations, int splitting, int max_blocks,
                       size_t master_block, uint8_t** out, size_t* out_len);
/* Test hooks (tests/ only): the match table of one input as Zopfli's sublen arrays — len16[i], dist16[i] and, when sublen
 * is not NULL, sublen[i * 259 + l] for l <= len16[i] — for block end `end` (0 = the input's end); and the length-limited
 * code lengths of one frequency vector (n <= 288, maxbits <= 15). */
int d4g_debug_zopfli_table(const uint8_t* raw, size_t n, size_t end, uint16_t* len16, uint16_t* dist16, uint16_t* sublen);
int d4g_debug_zopfli_code_lengths(const uint32_t* freq, int n, int maxbits, uint32_t* lengths);
/* Test hook (tests/ only): the header search's 19-symbol code-length trees (limit 7) of n histograms freq[h * 19 + s]:
 * lengths[h * 19 + s], and limited[h] = 1 where the tree was deeper than 7 and went through the depth limiter. */
int d4g_debug_cl_tree_lengths(const uint32_t* freq, int n, uint32_t* lengths, int32_t* limited);
/* Test hook (tests/ only): rewriteHeader(flags) of the code lengths lens320 = literal/length[288] + distance[32], of which the
 * first nLit and nDist count, packed by one wave as both search executors pack them: the RLE pairs (up to 320, encoded as
 * in d4g_types.h), their count, the 19 code-length-code lengths, nCl after trimming and the header's size in bits.
 * flags: bit 0 ohh, 1 use8, 2 use7, 3 alt8, 4 noRep, 5 noZRep, 6 noZRep2, 7 noRepZeros. */
int d4g_debug_pack_header(const uint8_t* lens320, int nLit, int nDist, int flags, uint16_t* pairs, int32_t* nPairs, uint8_t* clLen19, int32_t* nCl,
                          int32_t* bits);

#define D4G_MODE_NONE 0
#define D4G_MODE_CHEAP 1
#define D4G_MODE_ZOPFLI 2
#define D4G_MODE_ZOPFLI_EXTENSIVE 3
#define D4G_MODE_ZOPFLI_VERY_EXTENSIVE 4
/* CompressionUtil.compress(uncompressedData, threaded) (CompressionUtil.java:106-182) with useDeft = compareDeft = true
 * as CMDUtil configures it: every compressor output goes through Deft.optimiseDeflateStream(out, merge_blocks) and the
 * strict minimum by parsed bit size wins, ties to the earlier compressor in list order (the non-threaded loop :144-168 —
 * the threaded one takes completion order, which is not deterministic).  out[i] is always set; winner[i] (optional) is
 * the index of the winning output in list order. */
int d4g_compress(size_t n, const uint8_t* const* raw, const size_t* raw_len, int mode, int iter, int merge_blocks, uint8_t** out,
                 size_t* out_len, int32_t* winner);
/* CMDUtil.optimise for n raw deflate streams (CMDUtil.java:70-105): optimise; then, mode > NONE, recompress the decoded
 * bytes (d4g_compress), re-parse and optimise the winner, and take it iff its bit size is strictly smaller than the
 * optimised original's.  status[i]: D4G_STREAM_CHANGED (out[i] set: the optimised original or the grafted recompression),
 * D4G_STREAM_UNCHANGED (out[i] = NULL: keep the input), D4G_STREAM_PARSE_ERROR.  saved_bits[i] = DeflateStream.optimise's
 * return for the original; recompress_saved[i] = originalSize - recompSize when grafted, else 0. */
/* The same on a batch made by d4g_batch_create (inputs resident in HBM): afterwards d4g_batch_stream_result /
 * d4g_batch_copy_output describe the FINAL stream (the grafted recompression where it won); d4g_batch_recompress_result
 * tells which streams were grafted and by how many bits. */
int d4g_batch_run_recompress(d4g_batch* b, int mode, int iter, int merge_blocks);
int d4g_batch_recompress_result(d4g_batch* b, size_t i, int32_t* grafted, int64_t* recompress_saved);
int d4g_recompress_streams(size_t n, const uint8_t* const* in, const size_t* in_len, int mode, int iter, int merge_blocks,
                           uint8_t** out, size_t* out_len, int64_t* saved_bits, int64_t* recompress_saved, int32_t* status);

/* ---- round-trip verification: does what the library wrote decode to what it read? ----
 * d4g_batch_verify, valid after d4g_batch_run / _run_recompress / _run_encode: every stream whose final bytes the
 * library produced (status D4G_STREAM_CHANGED, a grafted recompression included; every output of an encoder batch) is
 * parsed again where it lies in HBM, the parse must read exactly out_len bytes and size_bits_in - saved_bits
 * (- recompress_saved) bits, and its decoded bytes are compared on the device with the batch's own decoded bytes of the
 * input (an encoder batch: the raw input).  No decoded byte goes through the host.  The call returns 0 when it could do
 * its work, whatever the verdicts.  first_mismatch: the byte offset for BYTES, the shorter length for LENGTH, else -1.
 * The checks run in the order PARSE, SIZE, BYTES, LENGTH: the compare covers the common prefix, so a differing byte
 * inside it is reported as BYTES even when the lengths differ too (bytes win over length).
 * d4g_verify_streams, usable on its own: do the raw DEFLATE streams a[i] and b[i] decode to the same bytes?  PARSE: b[i]
 * does not parse; SKIPPED: a[i] does not.  (No SIZE verdict: b[i] may be followed by other data.)
 * D4G_VERIFY=1 in the environment: every run call and every one-shot call that returns rewritten bytes verifies them
 * before it returns; a negative verdict makes the call fail with D4G_ERR_RUNTIME (d4g_last_error names the stream, the
 * verdict and the offset; a one-shot call hands back no buffers).  Unset or 0: no extra launch, no extra allocation. */
#define D4G_VERIFY_OK 0
#define D4G_VERIFY_SKIPPED 1      /* unchanged or unparsable input: the library wrote nothing */
#define D4G_VERIFY_PARSE (-1)
#define D4G_VERIFY_SIZE (-2)
#define D4G_VERIFY_LENGTH (-3)
#define D4G_VERIFY_BYTES (-4)
int d4g_batch_verify(d4g_batch* b);
int d4g_batch_verify_result(d4g_batch* b, size_t i, int32_t* verdict, int64_t* first_mismatch);
int d4g_verify_streams(size_t n, const uint8_t* const* a, const size_t* a_len, const uint8_t* const* b, const size_t* b_len,
                       int32_t* verdict, int64_t* first_mismatch);
/* Test hook (tests/ only): XORs xor_mask into byte byte_offset of stream i's final output in HBM after a run, so that a
 * test can show the verifier saying no.  It writes inside the stream's own output bytes only: any other offset is
 * D4G_ERR_ARG. */
int d4g_debug_batch_poke_output(d4g_batch* b, size_t i, size_t byte_offset, uint8_t xor_mask);
/* Test hook (tests/ only): the compare kernel alone on two host buffers of len bytes, placed x_skew and y_skew (0..15)
 * bytes past a 16-byte boundary of device memory: *first = offset of the first differing byte, -1 when they agree.
 * (Every decoded range the library itself compares starts on a 16-byte boundary; the kernel does not rely on it.) */
int d4g_debug_verify_compare(const uint8_t* x, size_t x_skew, const uint8_t* y, size_t y_skew, size_t len, int64_t* first);

/* Test hook (tests/ only): the static bin statistics of device block `block` of a batch (its Huffman blocks in stream
 * order; stored blocks have none), as k_block_bins left them.  A batch that has not run is parsed here the way
 * d4g_batch_run parses it (and then counts as run); d4g_batch_parse makes no tables, and a finished run has released them:
 * both give D4G_ERR_ARG "the block has no table", as does a block of an encoder batch.  table: 29 x 320 u32 (per length
 * symbol: byte counts, [256, 286) distance symbols, [286] records, [287] extra bits); masks: 29 x *mask_words u64, bit r
 * of a row set when record r carries that length symbol; records: *n_records x 4 u32 (x, y, z, w of every back-reference
 * record: packed length and symbols, offset of its bytes in the stream's decoded data, its first eight decoded bytes).
 * NULL buffers are skipped (the counts still come back); mask_cap / record_cap are in u64 words / records. */
int d4g_debug_batch_bins(d4g_batch* b, size_t block, uint32_t* table, uint64_t* masks, size_t mask_cap, uint32_t* records, size_t record_cap,
                         size_t* mask_words, size_t* n_records, size_t* n_blocks);

/* Debug and tests only: *live = device-memory blocks the pool of the calling thread's context (d4g_set_device) has handed
 * out and not yet got back.  Equal before and after any call — failed ones included — once the batches it made are closed. */
int d4g_debug_device_blocks(int64_t* live);

/* ---- per-block info: DeflateStream.printBlockInfo (B/deflate/DeflateStream.java:35-51) ----
 * which = 0: stream i as parsed (an encoder batch: as the encoder emitted it); 1: the final stream (the input's list
 * when the stream is unchanged; read off the written bytes otherwise, which verifies the batch if that has not happened).
 * bit_pos = position of the block's 3 header bits, size_bits = its size including them, as printBlockInfo counts them
 * (a stored block's padding follows its position); header_bits = a dynamic block's code-length header (else 0);
 * tokens includes the end-of-block symbol (0 for a stored block).  cap smaller than the count fills cap entries and
 * still sets *n_blocks. */
typedef struct d4g_block_info { int32_t type, bfinal; int64_t bit_pos, size_bits, header_bits, tokens, decoded_len; } d4g_block_info;
int d4g_batch_block_info(d4g_batch* b, size_t i, int which /* 0 = input as parsed, 1 = final stream */, d4g_block_info* out, size_t cap,
                         size_t* n_blocks);

/* ---- why a stream does not parse ----
 * The reference says "Failed to parse deflate stream data" and no more; here a stream that came back D4G_STREAM_PARSE_ERROR
 * can be asked where and why.  The answer is the first failure in token order, the one a sequential decoder stops at.
 * reason / bit_pos (first bit of the element that failed) / value (the offending value, -1 where there is none):
 *   OK                the stream parsed                                                       -1          -1
 *   EOF               the input ends inside an element: the 3 header bits (the empty input and a non-final last block
 *                     included), a stored block's LEN or NLEN, the 14 count bits, a code-length entry, any code or extra-bit
 *                     field                                  first bit of the field that could not be read in full   -1
 *   BLOCK_TYPE        BTYPE 3                                 the block's first header bit                 3
 *   STORED_LENGTHS    NLEN is not the complement of LEN       the byte-aligned position of LEN             LEN
 *   CODE_LENGTHS      no code-length code matches, a 16 with nothing before it, a run past HLIT + HDIST
 *                                                             first bit of the code-length symbol          the symbol, -1: no code
 *   LITLEN_SYMBOL     no literal/length code matches, or symbol 286 / 287      first bit of the token      the symbol, -1: no code
 *   DIST_SYMBOL       no distance code matches, or symbol 30 / 31              first bit of the token      the symbol, -1: no code
 *   DISTANCE_TOO_FAR  a back-reference reaches before the first decoded byte   first bit of the token      the distance
 *                     (a stream with a preset dictionary: before the dictionary's last 32 768 bytes)
 * block = blocks parsed before the failing one, block_bit_pos = its first header bit, decoded_offset = bytes of the whole
 * stream decoded before the failing element.  Whether a stream parses is decided by the parser alone; the diagnosis runs
 * only when asked (the first question about a batch diagnoses all its failed streams in one kernel launch and keeps the
 * answers), so a batch whose streams all parse never pays for it.  An encoder batch answers OK for every stream. */
#define D4G_PARSE_OK 0
#define D4G_PARSE_EOF 1
#define D4G_PARSE_BLOCK_TYPE 2
#define D4G_PARSE_STORED_LENGTHS 3
#define D4G_PARSE_CODE_LENGTHS 4
#define D4G_PARSE_LITLEN_SYMBOL 5
#define D4G_PARSE_DIST_SYMBOL 6
#define D4G_PARSE_DISTANCE_TOO_FAR 7
typedef struct d4g_parse_error {
    int32_t reason, block;          /* D4G_PARSE_*; index of the block that failed (-1 when OK) */
    int64_t block_bit_pos, bit_pos; /* the failing block's first header bit; the failing element's first bit */
    int64_t decoded_offset;         /* bytes decoded before the failing element */
    int64_t value;
} d4g_parse_error;
int d4g_batch_parse_error(d4g_batch* b, size_t i, d4g_parse_error* out);  /* after parse / run / run_recompress */
int d4g_diagnose_streams(size_t n, const uint8_t* const* in, const size_t* in_len, d4g_parse_error* out);
const char* d4g_parse_reason_name(int reason);  /* "OK", "EOF", "BLOCK_TYPE", ...; "UNKNOWN" for any other value; NULL before d4g_init */

/* ---- what decodes before the first failure ----
 * The recovered bytes R of stream i.  A stream that parses: its decoded bytes, exactly what d4g_batch_copy_decoded gives.  A
 * stream that does not: what a sequential decoder following the library's parser rule has produced when it meets the first
 * failure in token order — the decoded bytes of every block before the failing one, then those of the failing block's tokens
 * that precede the failing element.  The failing token contributes nothing (an invalid literal/length code; a length whose
 * distance code or extra bits fail or run out of input; a distance that reaches before the first decoded byte), and a failure
 * in a block's header (the 3 header bits, BTYPE 3, LEN / NLEN, the counts, the code lengths) contributes nothing of that
 * block.  len(R) == d4g_parse_error.decoded_offset always (0 included): the diagnosis decides where the failure is, recovery
 * decodes up to it.  (A stored block whose payload runs past the end of input parses, its missing bytes read as 0xff.)
 * Recovery runs only when asked: the first question decodes the leading bytes of all failed streams of the batch together, in
 * a side batch over the same device input, and keeps them until the batch is destroyed; a batch whose streams all parse
 * launches and allocates nothing.  Nothing else the batch reports changes, before or after a run, and
 * d4g_batch_copy_decoded still refuses a failed stream.  A prefix of 2 GiB or more is refused (D4G_ERR_RUNTIME).
 * Later intact members of a multi-member file are not pieced on: d4g_find_streams finds those. */
int d4g_batch_recover(d4g_batch* b);   /* after parse / run / run_recompress; idempotent; no failed stream: no work */
int d4g_batch_copy_recovered(d4g_batch* b, size_t i, uint8_t* dst, size_t cap, size_t* len);
    /* asks d4g_batch_recover itself; dst NULL: length only; a stream that parsed (and every stream of an encoder batch): as copy_decoded */
int d4g_recover_streams(size_t n, const uint8_t* const* in, const size_t* in_len, uint8_t** out, size_t* out_len,
                        d4g_parse_error* why /* may be NULL */);
    /* inflate as far as it goes: out[i] always set (d4g_free), why[i].reason == D4G_PARSE_OK for a stream that parsed;
     * on failure every out[i] is NULL, out_len[i] 0 and nothing is left allocated */

/* ---- embedded streams: where, in a file whose layout the library does not know, are the zlib and gzip streams? ----
 * (the reference's own wish list, deft4j-cmd/.../cmd/CMDUtil.java:120-125: "General support for optimising embedded GZip /
 * ZLib / deflate streams in other files".)  Every byte offset of every file is tested on the device; the survivors are
 * parsed, decoded and checked against their own trailer there, so a reported stream is wrong only when a 32-bit checksum
 * matches by accident.  What counts as a stream:
 *   zlib at offset o: o + 2 <= len; CMF = file[o], FLG = file[o+1]; (CMF & 15) == 8; (CMF >> 4) <= 7;
 *     (CMF * 256 + FLG) % 31 == 0; (FLG & 0x20) == 0.  The payload starts at o + 2.  The trailer is
 *     the 4 bytes right after the consumed payload, inside the file, big-endian, equal to the Adler-32 of the decoded bytes.
 *     With FDICT set ((FLG & 0x20) != 0) the header is a stream only for d4g_find_streams_dict, and only when o + 6 <= len and
 *     the four bytes after FLG (DICTID, big-endian) equal the Adler-32 of one of the caller's dictionaries, the first in list
 *     order: the payload then starts at o + 6, is parsed with that dictionary, total_len counts the 6 header bytes and
 *     `dictionary` reports 1 + the dictionary's index.  gzip has no dictionaries.
 *   gzip at offset o: the header bytes are 1f 8b 08 and FLG = file[o+3] has (FLG & 0xE0) == 0.  The 10 fixed header bytes
 *     are followed, in RFC 1952 order, by FEXTRA (XLEN, little-endian 16 bits, plus that many bytes), FNAME
 *     (zero-terminated), FCOMMENT (zero-terminated) and FHCRC (2 bytes, skipped and not checked — as
 *     containers.GZFile.read and K/GZFile.java:42-87 do).  All of these lie inside the file.  The trailer is the 8 bytes
 *     after the payload: CRC-32, little-endian, equal to that of the decoded bytes, then ISIZE, little-endian, equal to
 *     decoded_len mod 2^32.
 *   payload: it parses by the library's own parser rule, exactly as d4g_inflate would on file[payload_offset:], through a
 *     block with BFINAL set; no back-reference reaches before payload_offset (with FDICT: before the dictionary's last
 *     32 768 bytes, which lie in front of it); decoded_len >= min_decoded (default 0).
 *     Raw DEFLATE without a wrapper is not searched for: nothing confirms it.
 *   overlap: within a file, in ascending offset, a confirmed stream is reported iff offset >= the end (offset + total_len)
 *     of the last reported stream.  So a wrapper that lies inside another stream's compressed bytes, or inside its header
 *     or trailer, is not reported — a complete zlib stream carried verbatim in a stored block, for one.
 * Results are sorted by (file, offset); *found is released with d4g_free (NULL when nothing was found).  A file of 2 GiB or
 * more is refused with D4G_ERR_ARG.  A gzip FNAME / FCOMMENT is walked by one thread to its terminator. */
#define D4G_FOUND_ZLIB 1
#define D4G_FOUND_GZIP 2
typedef struct d4g_found_stream {
    int32_t file, kind;          /* index into the call's file list; D4G_FOUND_* */
    int64_t offset;              /* first byte of the wrapper's header */
    int64_t payload_offset;      /* first byte of the raw DEFLATE stream */
    int64_t payload_len;         /* bytes the parse consumed (d4g_inflate's *consumed) */
    int64_t total_len;           /* header + payload + trailer */
    int64_t decoded_len, size_bits;   /* size_bits = DeflateStream.getSizeBits */
    uint32_t crc32, adler32;     /* of the decoded bytes, both always filled */
    int32_t n_blocks, dictionary; /* dictionary: 0 none, else 1 + index of the preset dictionary (d4g_find_streams_dict) */
} d4g_found_stream;
typedef struct d4g_find_options { int32_t kinds /* OR of (1 << D4G_FOUND_*), 0 = all */, reserved; int64_t min_decoded; } d4g_find_options;
typedef struct d4g_find_stats {
    /* offsets tested; offsets whose header predicate held; of those, first block parsed; whole chain parsed; trailer
     * matched; reported after the overlap rule */
    int64_t bytes_scanned, header_candidates, first_block_ok, parsed, confirmed, reported, kernel_launches;
    double ms_total, ms_kernels; /* host wall clock of the call; device time of its kernels (HIP events) */
} d4g_find_stats;
int d4g_find_streams(size_t n, const uint8_t* const* file, const size_t* file_len, const d4g_find_options* opt /* NULL: defaults */,
                     d4g_found_stream** found /* d4g_free */, size_t* n_found, d4g_find_stats* stats /* may be NULL */);
/* d4g_find_streams plus zlib headers with FDICT whose DICTID names one of n_dict dictionaries; n_dict == 0: d4g_find_streams */
int d4g_find_streams_dict(size_t n, const uint8_t* const* file, const size_t* file_len, const d4g_find_options* opt, size_t n_dict,
                          const uint8_t* const* dict, const size_t* dict_len, d4g_found_stream** found, size_t* n_found, d4g_find_stats* stats);

/* ---- one-shot wrappers ----
 * Deft.optimiseDeflateStream for n streams: out[i]/out_len[i] are set only when status[i] ==
 * D4G_STREAM_CHANGED (else out[i] = NULL and the caller returns its original array). */
int d4g_optimise_streams(size_t n, const uint8_t* const* in, const size_t* in_len, int merge_blocks, uint8_t** out,
                         size_t* out_len, int64_t* saved_bits, int32_t* status);
/* The same list over every initialised context (d4g_init_devices): partitioned longest-first by compressed size, one host
 * thread and one device batch per context, no exchange between devices, outputs gathered in the caller's arrays in list order
 * (the C-level twin of deft4j_amd/shard.py; with one context it is d4g_optimise_streams). */
int d4g_optimise_streams_sharded(size_t n, const uint8_t* const* in, const size_t* in_len, int merge_blocks, uint8_t** out,
                                 size_t* out_len, int64_t* saved_bits, int32_t* status);
/* Deft.getSizeBitsFallback (B/Deft.java:48-54): parsed bit length, or len*8 when the stream does not parse */
int d4g_size_bits_fallback(const uint8_t* in, size_t len, int64_t* bits);
/* DeflateStream.parse + getUncompressedData; *consumed = bytes read.  Returns D4G_ERR_ARG-style <0 only on
 * library failure; *status receives D4G_STREAM_PARSE_ERROR for a malformed stream. */
int d4g_inflate(const uint8_t* in, size_t len, uint8_t** out, size_t* out_len, size_t* consumed, int32_t* status);
/* the same against a preset dictionary (d4g_batch_create_dict states the rule); dict_len 0: d4g_inflate */
int d4g_inflate_dict(const uint8_t* in, size_t len, const uint8_t* dict, size_t dict_len, uint8_t** out, size_t* out_len, size_t* consumed,
                     int32_t* status);
void d4g_free(void* p);

#ifdef __cplusplus
}
#endif
#endif /* DEFT4G_H */

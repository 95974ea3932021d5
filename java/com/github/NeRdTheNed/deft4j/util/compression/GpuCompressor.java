package com.github.NeRdTheNed.deft4j.util.compression;

import java.io.IOException;

import com.github.NeRdTheNed.deft4j.NativeDeft;

/**
 * A SingleCompressor (util/compression/SingleCompressor.java:6) backed by the MI355X LZ77 kernels: byte-identical to
 * JavaCompressor(strategy) for encoder ENC_JVM (zlib level 9; pinned by the asyoulik fixture), the jzlib restatement for
 * ENC_JZLIB.  CompressionUtil.getCompressors (CompressionUtil.java:44-78) would add
 *     new GpuCompressor(NativeDeft.ENC_JVM, Deflater.DEFAULT_STRATEGY) ...
 * in place of the JavaCompressor / JZLibCompressor entries, keeping the list order.  The three-argument constructor takes
 * a Deflater level (-1, 1..9; ENC_JVM only below 9) and also the strategies STRATEGY_RLE / STRATEGY_FIXED.
 */
public class GpuCompressor implements SingleCompressor {
    private final int encoder;
    private final int level;
    private final int strategy;
    private byte[] dictionary;

    public GpuCompressor(int encoder, int strategy) {
        this(encoder, 9, strategy);
    }

    public GpuCompressor(int encoder, int level, int strategy) {
        this.encoder = encoder;
        this.level = level;
        this.strategy = strategy;
    }

    /**
     * A preset dictionary in the manner of Deflater.setDictionary: every later compressSingle writes its stream against it
     * (raw DEFLATE; a reader needs the same dictionary).  null or an empty array: none.  ENC_JVM only.
     */
    public void setDictionary(byte[] dictionary) {
        this.dictionary = dictionary == null || dictionary.length == 0 ? null : dictionary.clone();
    }

    @Override
    public byte[] compressSingle(byte[] uncompressedData) throws IOException {
        if (dictionary != null) {
            return NativeDeft.deflateStreamsDict(new byte[][] { uncompressedData }, encoder, level, strategy, dictionary)[0];
        }
        if (level == 9 && strategy <= NativeDeft.STRATEGY_HUFFMAN_ONLY) {
            return NativeDeft.deflateStreams(new byte[][] { uncompressedData }, encoder, strategy)[0];
        }
        return NativeDeft.deflateStreamsLevel(new byte[][] { uncompressedData }, encoder, level, strategy)[0];
    }

    @Override
    public String getName() {
        return encoder == NativeDeft.ENC_JVM ? "GPU-zlib" : "GPU-jzlib";
    }
}

// The per-thread Huffman decoder of csrc/jpeg_dec.hip, in plain C++ so that a host program (tools/jpeg_dec_host_check.cpp, built with the
// host compiler's sanitizers) runs exactly what the kernels run.  Contract: README.md; CPU restatement: tests/_jpeg_dec_ref.py `Stream.run`.
//
// The stream is the unstuffed scan as big-endian bytes in 32-bit words, readable (zero) for 16 bytes past its end.  A decoder state is the
// triple (bit position, block slot within the MCU, zigzag index of the next coefficient; 0: the DC code is next).  `jd_run` decodes the
// symbols that START before `limit` and must keep going from a wrong state: a bit pattern that is no code skips one bit, a run past
// coefficient 63 ends the block, a symbol that would run over the end of the stream ends the decode at the end.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define JD_HD __host__ __device__ __forceinline__
#else
#define JD_HD inline
#endif

struct JdHuff {
    uint32_t lim[17];         // [l], l = 1..16: one past the largest code of length <= l, left-aligned in 16 bits (0..65536), nondecreasing
    int32_t valoff[17];       // [l]: index of the first value of length l minus the first code of length l
    uint8_t vals[256];
};

struct JdTables {
    JdHuff dc[2], ac[2];
};

struct JdState {
    uint32_t pos, slot, k;
};

struct JdScan {
    const uint32_t* words;    // the unstuffed stream, from its word `base_word` on (the kernels keep a workgroup's part in LDS)
    uint32_t base_word;
    uint32_t nbits;
    uint32_t nb;              // blocks per MCU
    uint32_t ny;              // of them luma (component 0); the next two are components 1 and 2
    uint32_t td_bits, ta_bits;    // bit c: the DC / AC table of component c (no indexed array: it would be promoted into LDS per thread)
};

// a DHT payload (16 counts, then the values) at file[off ..); every read is bounded by nbytes, a table that claims more than 256 values
// keeps the first 256
JD_HD void jd_build_huff(JdHuff& h, const uint8_t* file, uint32_t nbytes, uint32_t off) {
    int32_t code = 0, k = 0;
    h.lim[0] = 0, h.valoff[0] = 0;
    for (int l = 1; l <= 16; ++l) {
        const int32_t c = off + (uint32_t)l - 1u < nbytes ? (int32_t)file[off + l - 1] : 0;
        h.valoff[l] = k - code;
        k += c, code += c;
        // a 16-bit look-ahead v has a code of length <= l iff v < lim[l]; an over-full (malformed) table is clamped, so lim stays monotone
        uint64_t lim = c ? (uint64_t)(uint32_t)code << (16 - l) : (uint64_t)h.lim[l - 1];
        if (lim > 65536u) lim = 65536u;
        h.lim[l] = (uint32_t)lim > h.lim[l - 1] ? (uint32_t)lim : h.lim[l - 1];
        code <<= 1;
    }
    for (uint32_t i = 0; i < 256; ++i) h.vals[i] = ((int32_t)i < k && off + 16u + i < nbytes) ? file[off + 16u + i] : (uint8_t)0;
}

JD_HD uint32_t jd_bswap(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24); }

// the 32 bits from bit `pos` (pos < nbits: the two words are inside the stream or its zero padding)
JD_HD uint32_t jd_peek(const uint32_t* words, uint32_t base_word, uint32_t pos) {
    const uint32_t w = (pos >> 5) - base_word, s = pos & 31u;
    const uint64_t v = ((uint64_t)jd_bswap(words[w]) << 32) | jd_bswap(words[w + 1]);
    return (uint32_t)((v << s) >> 32);
}

// Sink: void operator()(uint32_t block, uint32_t zigzag_index, int value) -- DC differences and non-zero AC values of block `block`
template <class Sink>
JD_HD uint32_t jd_run(const JdScan& sc, const JdTables& t, JdState& st, uint32_t limit, uint32_t block, Sink&& sink) {
    uint32_t pos = st.pos, slot = st.slot, k = st.k, done = 0;
    if (limit > sc.nbits) limit = sc.nbits;
    while (pos < limit) {
        const uint32_t comp = slot < sc.ny ? 0u : slot - sc.ny + 1u;
        const JdHuff& h = k == 0 ? t.dc[(sc.td_bits >> comp) & 1u] : t.ac[(sc.ta_bits >> comp) & 1u];
        const uint32_t w = jd_peek(sc.words, sc.base_word, pos);
        // the code length without a data-dependent loop (lanes of a wave would all wait for the longest code): lim is monotone, so the
        // first l with v < lim[l] is one more than the number of l with v >= lim[l]
        const uint32_t v16 = w >> 16;
        uint32_t l = 1;
#ifdef __HIPCC__
#pragma unroll
#endif
        for (int i = 1; i <= 16; ++i) l += v16 >= h.lim[i] ? 1u : 0u;
        if (l > 16) {
            ++pos;
            continue;
        }
        const uint32_t c = w >> (32 - l);
        const uint32_t sym = h.vals[(uint32_t)(h.valoff[l] + (int32_t)c) & 255u];
        const uint32_t n = sym & 15u;
        if (pos + l + n > sc.nbits) {
            pos = sc.nbits;
            break;
        }
        int v = 0;
        if (n) {
            const uint32_t x = (w << l) >> (32 - n);
            v = x >= (1u << (n - 1)) ? (int)x : (int)x - (int)(1u << n) + 1;
        }
        pos += l + n;
        if (k == 0) {
            sink(block, 0u, v);
            k = 1;
        } else if (n == 0) {
            k = sym == 0xF0u ? k + 16 : 64;
        } else {
            k += sym >> 4;
            if (k < 64) sink(block, k, v);
            ++k;
        }
        if (k >= 64) {
            k = 0;
            slot = slot + 1 == sc.nb ? 0 : slot + 1;
            ++block, ++done;
        }
    }
    st.pos = pos, st.slot = slot, st.k = k;
    return done;
}

struct JdNoSink {
    JD_HD void operator()(uint32_t, uint32_t, int) const {}
};

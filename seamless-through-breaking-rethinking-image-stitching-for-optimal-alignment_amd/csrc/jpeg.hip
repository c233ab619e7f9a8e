// Baseline JPEG encoder for the result files of out.py (reference out.py:260-312 `to_pillow_fn(...).save(path)`): the file Pillow's
// `Image.save` writes at its defaults on libjpeg-turbo -- quality 75, 4:2:0 (RGB) or one component (L), Annex K Huffman tables, JFIF
// header, integer "islow" DCT -- byte for byte (contract: README.md; CPU restatement: tests/_jpeg_ref.py).  Integer arithmetic only.
//
//   jpeg_blocks_kernel  one wave per MCU (RGB: 16x16 px -> Y00 Y01 Y10 Y11 Cb Cr) or per 4 blocks of a block row (L): colour conversion,
//                       h2v2 downsampling, the edge / dummy-block rules, both DCT passes through LDS, quantisation -> int16 [nblocks, 64]
//                       zigzag coefficients in scan order
//   jpeg_bits_kernel    per block: DC difference (the predecessor is a closed-form index) and the block's code length in bits
//   jpeg_scan_kernel    exclusive prefix sum (one workgroup walking 4096-entry tiles) -> bit offset of every block, total
//   jpeg_zero_kernel    clears the words of the unstuffed stream that this image uses (part of the call: a reused workspace is fine)
//   jpeg_pack_kernel    per block: its codes at its bit offset (atomicOr on the two boundary words, plain stores between them); the
//                       last block appends the 1-bit padding
//   jpeg_count_kernel   0xFF bytes per 2048-byte chunk of the stream, scanned by jpeg_scan_kernel again
//   jpeg_stuff_kernel   scatters the bytes with their 0x00 followers behind the header; workgroup 0 writes the header (size bytes
//                       patched), EOI and the byte count
#include "common.h"
#include "jpeg_tables.h"

namespace {

// ---- tables (ITU-T T.81 Annex K: csrc/jpeg_tables.h), everything derived from them at compile time ----------------------------------
constexpr int kQuality = 75;

constexpr int kHdrMax = 624;
struct JTables {
    uint16_t q8[2][64];        // natural order: the divisor of the scaled-by-8 DCT output, quantiser << 3
    uint8_t izz[64];           // natural index -> zigzag position
    uint32_t dc[2][12];        // code | length << 16, index = category
    uint32_t ac[2][256];       // index = run << 4 | size
    uint8_t hdr[2][kHdrMax];   // SOI .. SOS; [0]: one component (L), [1]: RGB
    int32_t hdr_len[2];
    int32_t size_off[2];       // where SOF0's height (2 bytes) and width (2 bytes) go
};

constexpr int quantiser(int table, int natural) {
    const int scale = kQuality < 50 ? 5000 / kQuality : 200 - 2 * kQuality;
    const int q = (kQBase[table][natural] * scale + 50) / 100;
    return q < 1 ? 1 : (q > 255 ? 255 : q);
}

constexpr void huff_codes(uint32_t* tab, const int* bits, const int* vals, bool identity_vals) {
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i, ++k) tab[identity_vals ? k : vals[k]] = code++ | ((uint32_t)len << 16);
        code <<= 1;
    }
}

constexpr JTables make_tables() {
    JTables t{};
    for (int c = 0; c < 2; ++c)
        for (int i = 0; i < 64; ++i) t.q8[c][i] = (uint16_t)(quantiser(c, i) << 3);
    for (int i = 0; i < 64; ++i) t.izz[kZigzag[i]] = (uint8_t)i;
    for (int c = 0; c < 2; ++c) {
        huff_codes(t.dc[c], kDcBits[c], nullptr, true);
        huff_codes(t.ac[c], kAcBits[c], kAcVals[c], false);
    }
    for (int v = 0; v < 2; ++v) {
        const int ncomp = v ? 3 : 1, ntab = v ? 2 : 1;
        uint8_t* h = t.hdr[v];
        int n = 0;
        const uint8_t app0[20] = {0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
        for (int i = 0; i < 20; ++i) h[n++] = app0[i];
        for (int c = 0; c < ntab; ++c) {
            h[n++] = 0xFF, h[n++] = 0xDB, h[n++] = 0, h[n++] = 67, h[n++] = (uint8_t)c;
            for (int i = 0; i < 64; ++i) h[n++] = (uint8_t)quantiser(c, kZigzag[i]);
        }
        h[n++] = 0xFF, h[n++] = 0xC0, h[n++] = 0, h[n++] = (uint8_t)(8 + 3 * ncomp), h[n++] = 8;
        t.size_off[v] = n;
        n += 4;
        h[n++] = (uint8_t)ncomp;
        for (int c = 0; c < ncomp; ++c) h[n++] = (uint8_t)(c + 1), h[n++] = (v && c == 0) ? 0x22 : 0x11, h[n++] = c ? 1 : 0;
        for (int c = 0; c < ntab; ++c) {
            h[n++] = 0xFF, h[n++] = 0xC4, h[n++] = 0, h[n++] = 31, h[n++] = (uint8_t)c;
            for (int i = 0; i < 16; ++i) h[n++] = (uint8_t)kDcBits[c][i];
            for (int i = 0; i < 12; ++i) h[n++] = (uint8_t)i;
            h[n++] = 0xFF, h[n++] = 0xC4, h[n++] = 0, h[n++] = 181, h[n++] = (uint8_t)(0x10 | c);
            for (int i = 0; i < 16; ++i) h[n++] = (uint8_t)kAcBits[c][i];
            for (int i = 0; i < 162; ++i) h[n++] = (uint8_t)kAcVals[c][i];
        }
        h[n++] = 0xFF, h[n++] = 0xDA, h[n++] = 0, h[n++] = (uint8_t)(6 + 2 * ncomp), h[n++] = (uint8_t)ncomp;
        for (int c = 0; c < ncomp; ++c) h[n++] = (uint8_t)(c + 1), h[n++] = c ? 0x11 : 0x00;
        h[n++] = 0, h[n++] = 63, h[n++] = 0;
        t.hdr_len[v] = n;
    }
    return t;
}

constexpr JTables kTablesHost = make_tables();
static_assert(kTablesHost.hdr_len[0] == 328 && kTablesHost.hdr_len[1] == 623, "header sizes of the contract");
__device__ const JTables g_jt = make_tables();

// ---- sizes ------------------------------------------------------------------------------------------------------------------------
// A block codes to at most 20 + 63 * 26 bits: DC <= 20 (with the quality-75 quantisers a DC difference has at most 9 magnitude bits, and
// no DC code of either table is longer than 11), every AC coefficient <= 16 code bits + 10 magnitude bits; ZRL codes only replace
// coefficients.  Stuffing at most doubles the bytes.
constexpr uint32_t kMaxBlockBits = 20 + 63 * 26;
constexpr int64_t kMaxPixels = (int64_t)1 << 24;     // H * W limit: bit offsets stay below 2^32 (<= 442 k blocks * 1658 bits)
constexpr uint32_t kChunk = 2048;                    // stream bytes per workgroup of the stuffing pass (256 threads x 8 bytes)

struct JGeom {
    int32_t H, W, ch, stride;          // stride: bytes per canvas row
    int32_t mcu_cols, mcu_rows;        // RGB: 16x16 MCUs
    int32_t wib, hib;                  // 8x8 luma blocks per row / column (ceil)
    int32_t units;                     // waves of jpeg_blocks_kernel: MCUs (RGB) or groups of 4 blocks in a block row (L)
    uint32_t nblocks;
    uint32_t stream_words, nchunks;    // capacity of the unstuffed stream (32-bit words), of the chunk table
    size_t off_len, off_cnt, off_tot, off_stream, ws_bytes, out_bytes;
};

inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

bool make_geom(int32_t H, int32_t W, int32_t ch, JGeom& g) {
    if ((ch != 1 && ch != 3) || H < 1 || H > 65535 || W < 1 || W > 65535 || (int64_t)H * W > kMaxPixels) return false;
    g.H = H, g.W = W, g.ch = ch, g.stride = 0;
    g.mcu_cols = (W + 15) / 16, g.mcu_rows = (H + 15) / 16;
    g.wib = (W + 7) / 8, g.hib = (H + 7) / 8;
    if (ch == 3) {
        g.units = g.mcu_cols * g.mcu_rows;
        g.nblocks = 6u * (uint32_t)g.units;
    } else {
        g.units = g.hib * ((g.wib + 3) / 4);
        g.nblocks = (uint32_t)g.wib * (uint32_t)g.hib;
    }
    const uint64_t bits = (uint64_t)g.nblocks * kMaxBlockBits;
    const uint64_t bytes = (bits + 7) / 8;
    g.stream_words = (uint32_t)((bits + 31) / 32) + 4;
    g.nchunks = (uint32_t)((bytes + kChunk - 1) / kChunk);
    g.off_len = align16((size_t)g.nblocks * 128);
    g.off_cnt = g.off_len + align16((size_t)g.nblocks * 4);
    g.off_tot = g.off_cnt + align16((size_t)g.nchunks * 4);
    g.off_stream = g.off_tot + 16;
    g.ws_bytes = g.off_stream + align16((size_t)g.stream_words * 4);
    g.out_bytes = (size_t)kTablesHost.hdr_len[ch == 3] + 2 * (size_t)bytes + 2;
    return true;
}

// ---- kernel 1: canvas -> quantised blocks -----------------------------------------------------------------------------------------
constexpr int kWorkLd = 72;        // dwords per block of the row-pass output: 64 + 8, so the column pass of 4 blocks hits 32 distinct banks

template <int CH>
__global__ __launch_bounds__(256) void jpeg_blocks_kernel(const uint8_t* __restrict__ src, int16_t* __restrict__ coef, const JGeom g) {
    constexpr int NB = CH == 3 ? 6 : 4;
    __shared__ int16_t s_samp[4][NB * 64];
    __shared__ int16_t s_cbcr[4][CH == 3 ? 512 : 1];
    __shared__ int s_work[4][NB * kWorkLd];
    __shared__ __attribute__((aligned(4))) int16_t s_out[4][NB * 64];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int unit = blockIdx.x * 4 + wv;
    const bool live = unit < g.units;
    int16_t* samp = s_samp[wv];
    int* work = s_work[wv];
    int16_t* outc = s_out[wv];
    int ux = 0, uy = 0;            // RGB: MCU column / row; L: group of 4 blocks / block row
    if (live) {
        const int per_row = CH == 3 ? g.mcu_cols : (g.wib + 3) / 4;
        uy = unit / per_row, ux = unit - uy * per_row;
    }
    if (CH == 3) {
        int16_t* cbcr = s_cbcr[wv];
        if (live) {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int row = p * 4 + (lane >> 4), col = lane & 15;
                const int y = min(uy * 16 + row, g.H - 1), x = min(ux * 16 + col, g.W - 1);
                const uint8_t* px = src + (size_t)y * g.stride + (size_t)x * 3;
                const int r = px[0], gg = px[1], b = px[2];
                const int Y = (19595 * r + 38470 * gg + 7471 * b + 32768) >> 16;
                const int cb = (-11059 * r - 21709 * gg + 32768 * b + (128 << 16) + 32767) >> 16;
                const int cr = (32768 * r - 27439 * gg - 5329 * b + (128 << 16) + 32767) >> 16;
                samp[((row >> 3) * 2 + (col >> 3)) * 64 + (row & 7) * 8 + (col & 7)] = (int16_t)(Y - 128);
                cbcr[row * 16 + col] = (int16_t)cb;
                cbcr[256 + row * 16 + col] = (int16_t)cr;
            }
        }
        __syncthreads();
        if (live) {
            // h2v2: columns come from the (edge-replicated) input, rows past ceil(H / 2) replicate the last DOWNSAMPLED row
            const int cy = lane >> 3, cx = lane & 7;
            const int cyl = min(uy * 8 + cy, (g.H + 1) / 2 - 1) - uy * 8;
            const int bias = (cx & 1) ? 2 : 1;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int16_t* f = cbcr + c * 256 + (2 * cyl) * 16 + 2 * cx;
                samp[(4 + c) * 64 + lane] = (int16_t)(((f[0] + f[1] + f[16] + f[17] + bias) >> 2) - 128);
            }
        }
    } else {
        if (live) {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int row = p * 2 + (lane >> 5), col = lane & 31;
                const int y = min(uy * 8 + row, g.H - 1), x = min(ux * 32 + col, g.W - 1);
                samp[(col >> 3) * 64 + row * 8 + (col & 7)] = (int16_t)((int)src[(size_t)y * g.stride + x] - 128);
            }
        }
    }
    __syncthreads();
    const int blk = lane >> 3, rc = lane & 7;
    if (live && lane < NB * 8) {                                    // rows
        int d[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = samp[blk * 64 + rc * 8 + k];
        fdct8<true>(d);
#pragma unroll
        for (int k = 0; k < 8; ++k) work[blk * kWorkLd + rc * 8 + k] = d[k];
    }
    __syncthreads();
    if (live && lane < NB * 8) {                                    // columns, quantisation, zigzag
        int d[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = work[blk * kWorkLd + k * 8 + rc];
        fdct8<false>(d);
        const int t = (CH == 3 && blk >= 4) ? 1 : 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int nat = k * 8 + rc;
            const uint32_t q8 = g_jt.q8[t][nat];
            const uint32_t a = (uint32_t)abs(d[k]);
            const int r = (int)((a + (q8 >> 1)) / q8);
            outc[blk * 64 + g_jt.izz[nat]] = (int16_t)(d[k] < 0 ? -r : r);
        }
    }
    __syncthreads();
    if (!live) return;
    const uint32_t* out32 = (const uint32_t*)outc;
    uint32_t* dst = (uint32_t*)coef;
    if (CH == 3) {
        // a Y block its MCU needs past the image's blocks is a dummy: AC zero, DC of the block before it in the MCU (a dummy bottom
        // row: DC of the last block of the row above)
        const bool cdum = 2 * ux + 1 >= g.wib, rdum = 2 * uy + 1 >= g.hib;
        const uint32_t dc0 = (uint16_t)outc[0], dc1 = cdum ? dc0 : (uint16_t)outc[64], dc2 = rdum ? dc1 : (uint16_t)outc[128];
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            const int w = p * 64 + lane, b = w >> 5;
            uint32_t v = out32[w];
            if (b == 1 && cdum) v = (w & 31) ? 0u : dc0;
            if (b == 2 && rdum) v = (w & 31) ? 0u : dc1;
            if (b == 3 && (rdum || cdum)) v = (w & 31) ? 0u : (rdum ? dc1 : dc2);
            dst[(size_t)unit * 192 + w] = v;
        }
    } else {
        const size_t b0 = (size_t)uy * g.wib + (size_t)ux * 4;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int w = p * 64 + lane;
            if (ux * 4 + (w >> 5) < g.wib) dst[b0 * 32 + w] = out32[w];
        }
    }
}

// ---- entropy coding ---------------------------------------------------------------------------------------------------------------
struct HuffLds {
    uint32_t dc[2][12];
    uint32_t ac[2][256];
};

__device__ __forceinline__ void load_huff(HuffLds& h) {
    for (int i = threadIdx.x; i < 512; i += blockDim.x) h.ac[i >> 8][i & 255] = g_jt.ac[i >> 8][i & 255];
    if (threadIdx.x < 24) h.dc[threadIdx.x / 12][threadIdx.x % 12] = g_jt.dc[threadIdx.x / 12][threadIdx.x % 12];
    __syncthreads();
}

// scan-order predecessor of block b inside its component (-1: none) and the block's table (0 luma, 1 chroma)
__device__ __forceinline__ int64_t block_pred(uint32_t b, int ch, int& table) {
    table = 0;
    if (ch == 1) return (int64_t)b - 1;
    const uint32_t m = b / 6, j = b - m * 6;
    table = j >= 4;
    if (j >= 1 && j <= 3) return (int64_t)b - 1;
    if (m == 0) return -1;
    return (int64_t)(m - 1) * 6 + (j == 0 ? 3 : j);
}

__device__ __forceinline__ int coef_at(const uint4& w, int e) {      // e: constant after unrolling
    const uint32_t d = e < 2 ? w.x : e < 4 ? w.y : e < 6 ? w.z : w.w;
    return (int)(int16_t)((e & 1) ? (d >> 16) : (d & 0xffffu));
}

__device__ __forceinline__ int magnitude_bits(int v) { return 32 - __clz(abs(v)); }

__global__ __launch_bounds__(256) void jpeg_bits_kernel(const int16_t* __restrict__ coef, uint32_t* __restrict__ len, uint32_t nblocks, int ch) {
    __shared__ HuffLds h;
    load_huff(h);
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nblocks) return;
    int t;
    const int64_t pb = block_pred(b, ch, t);
    const int pred = pb < 0 ? 0 : (int)coef[pb * 64];
    const uint4* c4 = (const uint4*)(coef + (size_t)b * 64);
    uint32_t bits = 0;
    int run = 0;
#pragma unroll 1
    for (int q = 0; q < 8; ++q) {
        const uint4 w = c4[q];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int v = coef_at(w, e);
            if (q == 0 && e == 0) {
                const int n = magnitude_bits(v - pred);
                bits += (h.dc[t][n] >> 16) + n;
            } else if (v == 0) {
                ++run;
            } else {
                bits += (uint32_t)(run >> 4) * (h.ac[t][0xF0] >> 16);
                const int n = magnitude_bits(v);
                bits += (h.ac[t][((run & 15) << 4) | n] >> 16) + n;
                run = 0;
            }
        }
    }
    if (run) bits += h.ac[t][0] >> 16;
    len[b] = bits;
}

// in-place exclusive prefix sum of data[0 .. n), total -> *total.  One workgroup of 1024 threads, 4 entries per thread and tile.
// n = n_fixed, or, when total_bits is given, the number of kChunk-byte chunks of a stream of *total_bits bits.
__global__ __launch_bounds__(1024) void jpeg_scan_kernel(uint32_t* __restrict__ data, uint32_t n_fixed, const uint32_t* __restrict__ total_bits,
                                                         uint32_t* __restrict__ total) {
    __shared__ uint32_t s_wave[16];
    __shared__ uint32_t s_carry;
    uint32_t n = n_fixed;
    if (total_bits) n = min(n_fixed, (((*total_bits + 7u) >> 3) + kChunk - 1) / kChunk);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < n; base += 4096) {
        const uint32_t i0 = base + threadIdx.x * 4;
        uint32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = i0 + k < n ? data[i0 + k] : 0u;
        const uint32_t mine = v[0] + v[1] + v[2] + v[3];
        uint32_t inc = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = __shfl_up(inc, o, 64);
            if (lane >= o) inc += up;
        }
        if (lane == 63) s_wave[wv] = inc;
        __syncthreads();
        uint32_t before = s_carry;
        for (int k = 0; k < wv; ++k) before += s_wave[k];
        uint32_t run = before + inc - mine;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i0 + k < n) data[i0 + k] = run;
            run += v[k];
        }
        __syncthreads();
        if (threadIdx.x == 1023) s_carry = before + inc;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = s_carry;
}

__global__ __launch_bounds__(256) void jpeg_zero_kernel(uint32_t* __restrict__ stream, const uint32_t* __restrict__ total_bits, uint32_t cap_words) {
    const uint32_t words = min(cap_words, (*total_bits >> 5) + 4u);
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < words; i += gridDim.x * 256) stream[i] = 0u;
}

struct BitWriter {
    uint32_t* word;      // next word of the stream (bytes in stream order: the big-endian word, byte-swapped)
    uint64_t acc;        // pending bits in the low `n`
    int n;
    bool first;          // the next word is shared with the blocks before this one
};

__device__ __forceinline__ void put_bits(BitWriter& w, uint32_t v, int len) {
    w.acc = (w.acc << len) | v;
    w.n += len;
    if (w.n >= 32) {
        w.n -= 32;
        const uint32_t word = __builtin_bswap32((uint32_t)(w.acc >> w.n));
        if (w.first) atomicOr(w.word, word);
        else *w.word = word;
        w.first = false;
        ++w.word;
    }
}

__global__ __launch_bounds__(256) void jpeg_pack_kernel(const int16_t* __restrict__ coef, const uint32_t* __restrict__ off, const uint32_t* __restrict__ total_bits,
                                                        uint32_t* __restrict__ stream, uint32_t nblocks, int ch) {
    __shared__ HuffLds h;
    load_huff(h);
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nblocks) return;
    int t;
    const int64_t pb = block_pred(b, ch, t);
    const int pred = pb < 0 ? 0 : (int)coef[pb * 64];
    const uint4* c4 = (const uint4*)(coef + (size_t)b * 64);
    const uint32_t o = off[b];
    BitWriter w{stream + (o >> 5), 0, (int)(o & 31u), true};
    int run = 0;
#pragma unroll 1
    for (int q = 0; q < 8; ++q) {
        const uint4 cw = c4[q];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            int v = coef_at(cw, e);
            if (q == 0 && e == 0) {
                v -= pred;
                const int n = magnitude_bits(v);
                const uint32_t cl = h.dc[t][n];
                put_bits(w, ((cl & 0xffffu) << n) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1u)), (int)(cl >> 16) + n);
            } else if (v == 0) {
                ++run;
            } else {
                const uint32_t zrl = h.ac[t][0xF0];
                for (; run > 15; run -= 16) put_bits(w, zrl & 0xffffu, (int)(zrl >> 16));
                const int n = magnitude_bits(v);
                const uint32_t cl = h.ac[t][(run << 4) | n];
                put_bits(w, ((cl & 0xffffu) << n) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1u)), (int)(cl >> 16) + n);
                run = 0;
            }
        }
    }
    if (run) put_bits(w, h.ac[t][0] & 0xffffu, (int)(h.ac[t][0] >> 16));
    if (b == nblocks - 1) {                                           // the final partial byte is padded with 1-bits
        const int pad = (int)((8u - (*total_bits & 7u)) & 7u);
        put_bits(w, (1u << pad) - 1u, pad);
    }
    if (w.n > 0) atomicOr(w.word, __builtin_bswap32((uint32_t)(w.acc << (32 - w.n))));
}

__device__ __forceinline__ uint32_t block_sum_256(uint32_t v, uint32_t& exclusive, uint32_t* s_wave) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    if (lane == 63) s_wave[wv] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (int k = 0; k < 4; ++k) {
        if (k < wv) before += s_wave[k];
        all += s_wave[k];
    }
    exclusive = before + inc - v;
    return all;
}

__device__ __forceinline__ uint32_t ff_bytes(uint2 d, uint32_t i0, uint32_t nbytes) {
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t byte = ((k < 4 ? d.x : d.y) >> ((k & 3) * 8)) & 255u;
        c += (i0 + k < nbytes && byte == 255u) ? 1u : 0u;
    }
    return c;
}

__global__ __launch_bounds__(256) void jpeg_count_kernel(const uint32_t* __restrict__ stream, const uint32_t* __restrict__ total_bits, uint32_t* __restrict__ cnt) {
    __shared__ uint32_t s_wave[4];
    const uint32_t nbytes = (*total_bits + 7u) >> 3;
    if (blockIdx.x * kChunk >= nbytes) return;
    const uint32_t i0 = blockIdx.x * kChunk + threadIdx.x * 8;
    const uint2 d = i0 < nbytes ? *(const uint2*)(stream + (i0 >> 2)) : make_uint2(0u, 0u);
    uint32_t ex;
    const uint32_t all = block_sum_256(ff_bytes(d, i0, nbytes), ex, s_wave);
    if (threadIdx.x == 0) cnt[blockIdx.x] = all;
}

__global__ __launch_bounds__(256) void jpeg_stuff_kernel(const uint32_t* __restrict__ stream, const uint32_t* __restrict__ totals, const uint32_t* __restrict__ cnt_off,
                                                         uint8_t* __restrict__ out, int32_t* __restrict__ out_nbytes, int H, int W, int rgb) {
    __shared__ uint32_t s_wave[4];
    const uint32_t nbytes = (totals[0] + 7u) >> 3;
    const uint32_t hdr = (uint32_t)g_jt.hdr_len[rgb];
    if (blockIdx.x == 0) {
        const uint32_t so = (uint32_t)g_jt.size_off[rgb];
        for (uint32_t i = threadIdx.x; i < hdr; i += 256) {
            uint8_t v = g_jt.hdr[rgb][i];
            if (i == so) v = (uint8_t)(H >> 8);
            if (i == so + 1) v = (uint8_t)(H & 255);
            if (i == so + 2) v = (uint8_t)(W >> 8);
            if (i == so + 3) v = (uint8_t)(W & 255);
            out[i] = v;
        }
        if (threadIdx.x == 0) {
            const uint32_t end = hdr + nbytes + totals[1];
            out[end] = 0xFF, out[end + 1] = 0xD9;
            *out_nbytes = (int32_t)(end + 2);
        }
    }
    if (blockIdx.x * kChunk >= nbytes) return;
    const uint32_t i0 = blockIdx.x * kChunk + threadIdx.x * 8;
    const uint2 d = i0 < nbytes ? *(const uint2*)(stream + (i0 >> 2)) : make_uint2(0u, 0u);
    uint32_t ex;
    block_sum_256(ff_bytes(d, i0, nbytes), ex, s_wave);
    uint8_t* o = out + hdr + i0 + cnt_off[blockIdx.x] + ex;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t byte = ((k < 4 ? d.x : d.y) >> ((k & 3) * 8)) & 255u;
        if (i0 + k < nbytes) {
            *o++ = (uint8_t)byte;
            if (byte == 255u) *o++ = 0;
        }
    }
}

}  // namespace

// jpeg_scan_kernel for csrc/jpeg_dec.hip (its chunk and block counts): in-place exclusive prefix sum of data[0 .. n), total -> *total
hipError_t st_jpeg_scan_u32(uint32_t* data, uint32_t n, uint32_t* total, hipStream_t st) {
    hipLaunchKernelGGL(jpeg_scan_kernel, dim3(1), dim3(1024), 0, st, data, n, (const uint32_t*)nullptr, total);
    return hipGetLastError();
}

extern "C" int st_jpeg_workspace_bytes(int32_t H, int32_t W, int32_t channels) {
    JGeom g;
    return make_geom(H, W, channels, g) ? (int)g.ws_bytes : 0;
}

extern "C" int st_jpeg_max_bytes(int32_t H, int32_t W, int32_t channels) {
    JGeom g;
    return make_geom(H, W, channels, g) ? (int)g.out_bytes : 0;
}

extern "C" int st_jpeg_encode_u8(const void* src, int32_t H, int32_t W, int32_t channels, int64_t row_stride, void* out, int64_t out_capacity,
                                 int32_t* out_nbytes, void* workspace, int64_t workspace_bytes, void* stream) {
    JGeom g;
    if (!src || !out || !out_nbytes || !workspace || !make_geom(H, W, channels, g)) return ST_EINVAL;
    if (row_stride < (int64_t)W * channels || row_stride > 0x7fffffff || ((uintptr_t)workspace & 15)) return ST_EINVAL;
    if (out_capacity < (int64_t)g.out_bytes || workspace_bytes < (int64_t)g.ws_bytes) return ST_EINVAL;
    g.stride = (int32_t)row_stride;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    int16_t* coef = (int16_t*)ws;
    uint32_t* len = (uint32_t*)(ws + g.off_len);
    uint32_t* cnt = (uint32_t*)(ws + g.off_cnt);
    uint32_t* tot = (uint32_t*)(ws + g.off_tot);          // [0] bits of the scan, [1] its 0xFF bytes
    uint32_t* bits = (uint32_t*)(ws + g.off_stream);
    const unsigned per_block = (g.nblocks + 255) / 256;
    if (channels == 3)
        hipLaunchKernelGGL(jpeg_blocks_kernel<3>, dim3((g.units + 3) / 4), dim3(256), 0, st, (const uint8_t*)src, coef, g);
    else
        hipLaunchKernelGGL(jpeg_blocks_kernel<1>, dim3((g.units + 3) / 4), dim3(256), 0, st, (const uint8_t*)src, coef, g);
    ST_CHECK_LAUNCH();
    hipLaunchKernelGGL(jpeg_bits_kernel, dim3(per_block), dim3(256), 0, st, (const int16_t*)coef, len, g.nblocks, channels);
    ST_CHECK_LAUNCH();
    hipLaunchKernelGGL(jpeg_scan_kernel, dim3(1), dim3(1024), 0, st, len, g.nblocks, (const uint32_t*)nullptr, tot);
    ST_CHECK_LAUNCH();
    const unsigned zero_grid = (g.stream_words + 255) / 256 < 512 ? (g.stream_words + 255) / 256 : 512;
    hipLaunchKernelGGL(jpeg_zero_kernel, dim3(zero_grid), dim3(256), 0, st, bits, (const uint32_t*)tot, g.stream_words);
    ST_CHECK_LAUNCH();
    hipLaunchKernelGGL(jpeg_pack_kernel, dim3(per_block), dim3(256), 0, st, (const int16_t*)coef, (const uint32_t*)len, (const uint32_t*)tot, bits, g.nblocks,
                       channels);
    ST_CHECK_LAUNCH();
    hipLaunchKernelGGL(jpeg_count_kernel, dim3(g.nchunks), dim3(256), 0, st, (const uint32_t*)bits, (const uint32_t*)tot, cnt);
    ST_CHECK_LAUNCH();
    hipLaunchKernelGGL(jpeg_scan_kernel, dim3(1), dim3(1024), 0, st, cnt, g.nchunks, (const uint32_t*)tot, tot + 1);
    ST_CHECK_LAUNCH();
    hipLaunchKernelGGL(jpeg_stuff_kernel, dim3(g.nchunks), dim3(256), 0, st, (const uint32_t*)bits, (const uint32_t*)tot, (const uint32_t*)cnt, (uint8_t*)out,
                       out_nbytes, H, W, channels == 3 ? 1 : 0);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

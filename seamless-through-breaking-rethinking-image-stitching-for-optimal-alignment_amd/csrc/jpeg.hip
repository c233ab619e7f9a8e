// Baseline JPEG encoder for the result files of out.py (reference out.py:260-312 `to_pillow_fn(...).save(path)`): the file Pillow's
// `Image.save(path, quality=q, subsampling=s, optimize=o)` writes on libjpeg-turbo -- JFIF header, integer "islow" DCT, 4:2:0 / 4:2:2 /
// 4:4:4 (RGB) or one component (L), the Annex K Huffman tables or libjpeg's optimised ones -- byte for byte (contract: README.md; CPU
// restatements: tests/_jpeg_ref.py for Pillow's defaults, tests/_jpeg_opts_ref.py for the keywords).  One kernel set serves both C entries:
// st_jpeg_encode_u8 is st_jpeg_encode_u8_ex at {75, 4:2:0 or one component, plain}.  The quantisers are kernel arguments, the sampling a
// template parameter and the code tables memory: the Annex K ones (g_std), or the ones the table kernel has just made from the image's own
// symbol counts.  Integer arithmetic only.
//
//   jpeg_blocks_kernel  one wave per MCU (4:2:0 16x16: Y00 Y01 Y10 Y11 Cb Cr; 4:2:2 16x8: Y0 Y1 Cb Cr; 4:4:4 8x8: Y Cb Cr) or per 4 blocks
//                       of a block row (L): colour conversion, h2v2 / h2v1 downsampling, the edge and dummy-block rules, both DCT passes
//                       through LDS, quantisation -> int16 [nblocks, 64] zigzag coefficients in scan order; (optimize) workgroup 0 clears the
//                       histograms
//   jpeg_hist_kernel    (optimize) the symbols the scan will emit, ZRL and EOB included, counted in LDS per workgroup, merged into
//                       uint32 [4][257]: DC0, AC0, DC1, AC1
//   jpeg_table_kernel   (optimize) one wave per table: jpeg_gen_optimal_table (csrc/jpeg_huff_core.h) -> code | length per symbol and the
//                       DHT payload with its length
//   jpeg_bits_kernel    per block: DC difference (the predecessor is a closed-form index) and the block's code length in bits, with the
//                       tables in LDS
//   jpeg_scan_kernel    exclusive prefix sum (one workgroup walking 4096-entry tiles) -> bit offset of every block, total
//   jpeg_zero_kernel    clears the words of the unstuffed stream that this image uses (part of the call: a reused workspace is fine)
//   jpeg_pack_kernel    per block: its codes at its bit offset (atomicOr on the two boundary words, plain stores between them); the
//                       last block appends the 1-bit padding
//   jpeg_count_kernel   0xFF bytes per 2048-byte chunk of the stream, scanned by jpeg_scan_kernel again
//   jpeg_stuff_kernel   scatters the bytes with their 0x00 followers behind the header; the last workgroup assembles the header -- DQT from
//                       the arguments, SOF0, the DHTs of fixed or device-computed length -- and writes EOI and the byte count
#include "common.h"
#include "jpeg_tables.h"
#include "jpeg_huff_core.h"
#include "jpeg_scan.h"
#include "jpeg_enc_core.h"
#include "jpeg_rst.h"
#include "../../include/stitch_gfx950.h"

namespace {

__device__ const JIzz g_izz = make_izz();

struct JQuant {
    uint16_t q8[2][64];                // natural order: the divisor of the scaled-by-8 DCT output, quantiser << 3
};

// ---- sizes ------------------------------------------------------------------------------------------------------------------------
// A block codes to fewer than 20 + 63 * 26 bits with ANY table of codes <= 16 bits: a coefficient of s magnitude bits is at least
// 2^(s-1) quantiser steps, the squares of a block's 64 DCT outputs sum to at most 64 * 128^2 = 2^20 (the transform is orthonormal up to its
// rounding), so 63 AC coefficients can average at most 8 magnitude bits: 63 * (16 + 8) + (16 + 11) = 1539 bits.  Stuffing at most doubles
// the bytes.
constexpr uint32_t kMaxBlockBits = 20 + 63 * 26;
constexpr int64_t kMaxPixels = (int64_t)1 << 24;     // H * W limit: bit offsets stay below 2^32 (<= 3 * 2^18 blocks * 1658 bits)
constexpr uint32_t kChunk = 2048;                    // stream bytes per workgroup of the stuffing pass (256 threads x 8 bytes)
constexpr int kWorkLd = 72;        // dwords per block of the row-pass output: 64 + 8, so the column pass of 4 blocks hits 32 distinct banks

struct JGeom {
    int32_t H, W, ch, stride;          // stride: bytes per canvas row
    int32_t mcu_cols, mcu_rows;
    int32_t wib, hib;                  // 8x8 luma blocks per row / column (ceil)
    int32_t units;                     // waves of jpeg_blocks_kernel: MCUs (RGB) or groups of 4 blocks in a block row (L)
    int32_t nb, ny;                    // blocks per MCU, of them luma
    uint32_t nblocks;
    uint32_t stream_words, nchunks;    // capacity of the unstuffed stream (32-bit words), of the chunk table
    size_t off_len, off_cnt, off_tot, off_dev, off_stream, ws_bytes, out_bytes;
};

inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// restart intervals (reserved[0] = Ri MCUs > 0, csrc/jpeg_rst.hip): n = ceil(MCUs / Ri) intervals.  Each adds at most 7 padding bits to the
// stream (counted as a byte, doubled like every byte for stuffing: 2 bytes of the file) and one two-byte marker; the DRI segment is 6 bytes.
// The workspace grows by the stream's share of that and by two tables of n + 1 words behind the stream.
struct JRstGeom {
    uint32_t ri, nint;
    size_t off_pad, off_ibyte;
};

bool make_geom(int32_t H, int32_t W, int32_t ch, const st_jpeg_enc_params* p, JGeom& g, JRstGeom* rst = nullptr) {
    if (!p || (ch != 1 && ch != 3) || H < 1 || H > 65535 || W < 1 || W > 65535 || (int64_t)H * W > kMaxPixels) return false;
    if (p->quality < 1 || p->quality > 100 || (p->optimize != 0 && p->optimize != 1)) return false;
    if (!((p->hs == 1 && p->vs == 1) || (ch == 3 && p->hs == 2 && (p->vs == 1 || p->vs == 2)))) return false;
    if (p->reserved[0] < 0 || p->reserved[0] > 65535 || p->reserved[1] || p->reserved[2] || p->reserved[3]) return false;
    g.H = H, g.W = W, g.ch = ch, g.stride = 0;
    g.mcu_cols = (W + 8 * p->hs - 1) / (8 * p->hs), g.mcu_rows = (H + 8 * p->vs - 1) / (8 * p->vs);
    g.wib = (W + 7) / 8, g.hib = (H + 7) / 8;
    if (ch == 3) {
        g.ny = p->hs * p->vs, g.nb = g.ny + 2;
        g.units = g.mcu_cols * g.mcu_rows;
        g.nblocks = (uint32_t)g.nb * (uint32_t)g.units;
    } else {
        g.ny = 1, g.nb = 1;
        g.units = g.hib * ((g.wib + 3) / 4);
        g.nblocks = (uint32_t)g.wib * (uint32_t)g.hib;
    }
    const uint32_t ri = (uint32_t)p->reserved[0], nmcu = g.nblocks / (uint32_t)g.nb, nint = ri ? (nmcu + ri - 1) / ri : 0u;
    const uint64_t bits = (uint64_t)g.nblocks * kMaxBlockBits + 8u * (uint64_t)nint;
    const uint64_t bytes = (bits + 7) / 8;
    g.stream_words = (uint32_t)((bits + 31) / 32) + 4;
    g.nchunks = (uint32_t)((bytes + kChunk - 1) / kChunk);
    g.off_len = align16((size_t)g.nblocks * 128);
    g.off_cnt = g.off_len + align16((size_t)g.nblocks * 4);
    g.off_tot = g.off_cnt + align16((size_t)g.nchunks * 4);
    g.off_dev = g.off_tot + 16;
    g.off_stream = g.off_dev + (p->optimize ? align16(sizeof(JDev)) : 0);      // the plain path has no table area and reads none
    g.ws_bytes = g.off_stream + align16((size_t)g.stream_words * 4);
    const size_t off_pad = g.ws_bytes, off_ibyte = off_pad + align16((size_t)(nint + 1) * 4);
    if (ri) g.ws_bytes = off_ibyte + align16((size_t)(nint + 1) * 4);
    if (rst) *rst = JRstGeom{ri, nint, off_pad, off_ibyte};
    g.out_bytes = (size_t)kStdHeaderBytes[ch == 3] + (ri ? 6u : 0u) + 2 * (size_t)bytes + 2 * (size_t)nint + 2;
    return g.ws_bytes <= 0x7fffffffu && g.out_bytes <= 0x7fffffffu;
}

// ---- kernel 1: canvas -> quantised blocks -----------------------------------------------------------------------------------------
template <int CH, int HS, int VS>
__global__ __launch_bounds__(256) void jpeg_blocks_kernel(const uint8_t* __restrict__ src, int16_t* __restrict__ coef, const JGeom g, const JQuant qt,
                                                          uint32_t* __restrict__ hist) {
    constexpr int NY = CH == 3 ? HS * VS : 4, NB = CH == 3 ? NY + 2 : 4;
    constexpr int MW = 8 * HS, MH = 8 * VS;
    __shared__ int16_t s_samp[4][NB * 64];
    __shared__ int16_t s_cbcr[4][(CH == 3 && HS == 2) ? 2 * MW * MH : 1];
    __shared__ int s_work[4][NB * kWorkLd];
    __shared__ __attribute__((aligned(4))) int16_t s_out[4][NB * 64];
    if (hist && blockIdx.x == 0)
        for (int i = threadIdx.x; i < 4 * kJhEntries; i += 256) hist[i] = 0u;
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
            for (int p = 0; p < HS * VS; ++p) {
                const int idx = p * 64 + lane, row = idx / MW, col = idx % MW;
                const int y = min(uy * MH + row, g.H - 1), x = min(ux * MW + col, g.W - 1);
                const uint8_t* px = src + (size_t)y * g.stride + (size_t)x * 3;
                const int r = px[0], gg = px[1], b = px[2];
                const int Y = (19595 * r + 38470 * gg + 7471 * b + 32768) >> 16;
                const int cb = (-11059 * r - 21709 * gg + 32768 * b + (128 << 16) + 32767) >> 16;
                const int cr = (32768 * r - 27439 * gg - 5329 * b + (128 << 16) + 32767) >> 16;
                samp[((row >> 3) * HS + (col >> 3)) * 64 + (row & 7) * 8 + (col & 7)] = (int16_t)(Y - 128);
                if (HS == 1) {                                      // 4:4:4: chroma is copied
                    samp[64 + idx] = (int16_t)(cb - 128);
                    samp[128 + idx] = (int16_t)(cr - 128);
                } else {
                    cbcr[row * MW + col] = (int16_t)cb;
                    cbcr[MW * MH + row * MW + col] = (int16_t)cr;
                }
            }
        }
        if (HS == 2) {
            __syncthreads();
            if (live) {
                const int cy = lane >> 3, cx = lane & 7;
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    if (VS == 2) {
                        // h2v2: columns come from the (edge-replicated) input, rows past ceil(H / 2) replicate the last DOWNSAMPLED row
                        const int cyl = min(uy * 8 + cy, (g.H + 1) / 2 - 1) - uy * 8;
                        const int16_t* f = cbcr + c * 256 + (2 * cyl) * 16 + 2 * cx;
                        samp[(4 + c) * 64 + lane] = (int16_t)(((f[0] + f[1] + f[16] + f[17] + ((cx & 1) ? 2 : 1)) >> 2) - 128);
                    } else {
                        // h2v1: the same column rule; the bias alternates 0, 1 over the output columns
                        const int16_t* f = cbcr + c * 128 + cy * 16 + 2 * cx;
                        samp[(2 + c) * 64 + lane] = (int16_t)(((f[0] + f[1] + (cx & 1)) >> 1) - 128);
                    }
                }
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
        const int t = (CH == 3 && blk >= NY) ? 1 : 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int nat = k * 8 + rc;
            const uint32_t q8 = qt.q8[t][nat];
            const uint32_t a = (uint32_t)abs(d[k]);
            const int r = (int)((a + (q8 >> 1)) / q8);
            outc[blk * 64 + g_izz.v[nat]] = (int16_t)(d[k] < 0 ? -r : r);
        }
    }
    __syncthreads();
    if (!live) return;
    const uint32_t* out32 = (const uint32_t*)outc;
    uint32_t* dst = (uint32_t*)coef;
    if (CH == 3) {
        // a Y block its MCU needs past the image's blocks is a dummy: AC zero, DC of the block before it in the MCU (a dummy bottom
        // row: DC of the last block of the row above)
        const bool cdum = HS == 2 && 2 * ux + 1 >= g.wib, rdum = VS == 2 && 2 * uy + 1 >= g.hib;
        const uint32_t dc0 = (uint16_t)outc[0], dc1 = cdum ? dc0 : (uint16_t)outc[64], dc2 = rdum ? dc1 : (uint16_t)outc[128];
#pragma unroll
        for (int p = 0; p < (NB + 1) / 2; ++p) {
            const int w = p * 64 + lane, b = w >> 5;
            if (w < NB * 32) {
                uint32_t v = out32[w];
                if (b == 1 && cdum) v = (w & 31) ? 0u : dc0;
                if (VS == 2 && b == 2 && rdum) v = (w & 31) ? 0u : dc1;
                if (VS == 2 && b == 3 && (rdum || cdum)) v = (w & 31) ? 0u : (rdum ? dc1 : dc2);
                dst[(size_t)unit * (NB * 32) + w] = v;
            }
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
__global__ __launch_bounds__(256) void jpeg_hist_kernel(const int16_t* __restrict__ coef, uint32_t* __restrict__ hist, uint32_t nblocks, uint32_t nb, uint32_t ny) {
    __shared__ uint32_t s_hist[4 * kJhEntries];
    for (int i = threadIdx.x; i < 4 * kJhEntries; i += 256) s_hist[i] = 0u;
    __syncthreads();
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b < nblocks) {
        int t;
        const int64_t pb = block_pred(b, nb, ny, t);
        const int pred = pb < 0 ? 0 : (int)coef[pb * 64];
        uint32_t* hd = s_hist + (2 * t) * kJhEntries;
        uint32_t* ha = hd + kJhEntries;
        walk_block(
            coef, b, pred, [&](int n, int) { atomicAdd(hd + (n & 15), 1u); },
            [&](int k) {
                if (k) atomicAdd(ha + 0xF0, (uint32_t)k);
            },
            [&](int sym, int, int) { atomicAdd(ha + (sym & 255), 1u); });
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 4 * kJhEntries; i += 256) {
        const uint32_t v = s_hist[i];
        if (v) atomicAdd(hist + i, v);
    }
}

struct WaveTeam {
    static constexpr int LANES = 64;
    __device__ __forceinline__ int lane() const { return (int)threadIdx.x; }
    __device__ __forceinline__ static uint64_t xor64(uint64_t v, int o) {
        return ((uint64_t)__shfl_xor((uint32_t)(v >> 32), o, 64) << 32) | __shfl_xor((uint32_t)v, o, 64);
    }
    __device__ __forceinline__ void min2_u64(uint64_t& a, uint64_t& b) const {      // butterfly: partners merge disjoint sets of lanes
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint64_t pa = xor64(a, o), pb = xor64(b, o);
            const uint64_t lo = a < pa ? a : pa, hi = a < pa ? pa : a, rest = b < pb ? b : pb;
            a = lo, b = hi < rest ? hi : rest;
        }
    }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
};

__global__ __launch_bounds__(64) void jpeg_table_kernel(JDev* __restrict__ dev) {
    __shared__ JhWork s;
    const int t = blockIdx.x;
    jh_gen_optimal_table(WaveTeam{}, dev->hist[t], s);
    JTabs& o = dev->tabs;
    for (int i = threadIdx.x; i < 256; i += 64) {
        o.code[t][i] = s.code[i];
        o.dht[t][16 + i] = i < s.nsym ? s.huffval[i] : (uint8_t)0;
    }
    if (threadIdx.x < 16) o.dht[t][threadIdx.x] = (uint8_t)s.bits[threadIdx.x + 1];
    if (threadIdx.x == 0) o.dht_len[t] = 16 + s.nsym;
}

// dev: the tables the table kernel made, or nullptr for the Annex K ones (here and below)
__global__ __launch_bounds__(256) void jpeg_bits_kernel(const int16_t* __restrict__ coef, uint32_t* __restrict__ len, const JDev* __restrict__ dev, uint32_t nblocks,
                                                        uint32_t nb, uint32_t ny) {
    __shared__ HuffLds h;
    load_huff(h, dev ? &dev->tabs : &g_std);
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nblocks) return;
    int t;
    const int64_t pb = block_pred(b, nb, ny, t);
    const int pred = pb < 0 ? 0 : (int)coef[pb * 64];
    uint32_t bits = 0;
    walk_block(
        coef, b, pred, [&](int n, int) { bits += (h.dc[t][n & 15] >> 16) + n; }, [&](int k) { bits += (uint32_t)k * (h.ac[t][0xF0] >> 16); },
        [&](int sym, int, int n) { bits += (h.ac[t][sym & 255] >> 16) + n; });
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

__global__ __launch_bounds__(256) void jpeg_pack_kernel(const int16_t* __restrict__ coef, const uint32_t* __restrict__ off, const uint32_t* __restrict__ total_bits,
                                                        uint32_t* __restrict__ stream, uint32_t cap_words, const JDev* __restrict__ dev, uint32_t nblocks, uint32_t nb,
                                                        uint32_t ny) {
    __shared__ HuffLds h;
    load_huff(h, dev ? &dev->tabs : &g_std);
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nblocks) return;
    int t;
    const int64_t pb = block_pred(b, nb, ny, t);
    const int pred = pb < 0 ? 0 : (int)coef[pb * 64];
    const uint32_t o = off[b];
    BitWriter w{stream + (o >> 5), stream + cap_words, 0, (int)(o & 31u), true};
    auto put = [&](uint32_t cl, int v, int n) {
        put_bits(w, ((cl & 0xffffu) << n) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1u)), (int)(cl >> 16) + n);
    };
    walk_block(
        coef, b, pred, [&](int n, int v) { put(h.dc[t][n & 15], v, n); },
        [&](int k) {
            for (; k > 0; --k) put(h.ac[t][0xF0], 0, 0);
        },
        [&](int sym, int v, int n) { put(h.ac[t][sym & 255], v, n); });
    if (b == nblocks - 1) {                                           // the final partial byte is padded with 1-bits
        const int pad = (int)((8u - (*total_bits & 7u)) & 7u);
        put_bits(w, (1u << pad) - 1u, pad);
    }
    if (w.n > 0 && w.word < w.end) atomicOr(w.word, __builtin_bswap32((uint32_t)(w.acc << (32 - w.n))));
}

// chunks behind the stream get no count: jpeg_scan_kernel bounds itself with the same total_bits
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
                                                         uint8_t* __restrict__ out, int32_t* __restrict__ out_nbytes, const JHeader hp, const JDev* __restrict__ dev) {
    __shared__ uint32_t s_wave[4];
    const JTabs* tabs = dev ? &dev->tabs : &g_std;
    const uint32_t nbytes = (totals[0] + 7u) >> 3;
    const uint32_t hdr = dev ? header_bytes(hp.ncomp, dev->tabs) : hp.std_bytes;
    // the header is the last workgroup's: its chunk lies behind the stream unless the image fills the worst case, so the header is written
    // beside the scatter and not in front of workgroup 0's
    if (blockIdx.x == gridDim.x - 1) {
        write_header(out, hp, tabs);
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

int quantiser(int table, int natural, int quality) {                 // jpeg_quality_scaling + jpeg_add_quant_table, baseline clamp
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int q = (kQBase[table][natural] * scale + 50) / 100;
    return q < 1 ? 1 : (q > 255 ? 255 : q);
}

st_jpeg_enc_params default_params(int32_t channels) {                // Pillow's defaults: quality 75, 4:2:0 (one channel: 1 x 1), Annex K tables
    const int32_t s = channels == 3 ? 2 : 1;
    return st_jpeg_enc_params{75, s, s, 0, {0, 0, 0, 0}};
}

}  // namespace

hipError_t st_jpeg_scan_u32(uint32_t* data, uint32_t n, uint32_t* total, hipStream_t st) {
    hipLaunchKernelGGL(jpeg_scan_kernel, dim3(1), dim3(1024), 0, st, data, n, (const uint32_t*)nullptr, total);
    return hipGetLastError();
}

extern "C" int st_abi_jpeg_enc_params_size(void) { return (int)sizeof(st_jpeg_enc_params); }

extern "C" int st_jpeg_workspace_bytes_ex(int32_t H, int32_t W, int32_t channels, const st_jpeg_enc_params* params) {
    JGeom g;
    return make_geom(H, W, channels, params, g) ? (int)g.ws_bytes : 0;
}

extern "C" int st_jpeg_max_bytes_ex(int32_t H, int32_t W, int32_t channels, const st_jpeg_enc_params* params) {
    JGeom g;
    return make_geom(H, W, channels, params, g) ? (int)g.out_bytes : 0;
}

extern "C" int st_jpeg_encode_u8_ex(const void* src, int32_t H, int32_t W, int32_t channels, int64_t row_stride, const st_jpeg_enc_params* params, void* out,
                                    int64_t out_capacity, int32_t* out_nbytes, void* workspace, int64_t workspace_bytes, void* stream) {
    JGeom g;
    JRstGeom rg;
    if (!src || !out || !out_nbytes || !workspace || !make_geom(H, W, channels, params, g, &rg)) return ST_EINVAL;
    if (row_stride < (int64_t)W * channels || row_stride > 0x7fffffff || ((uintptr_t)workspace & 15)) return ST_EINVAL;
    if (out_capacity < (int64_t)g.out_bytes || workspace_bytes < (int64_t)g.ws_bytes) return ST_EINVAL;
    g.stride = (int32_t)row_stride;
    JQuant qt;
    JHeader hp;
    hp.H = H, hp.W = W, hp.ncomp = channels, hp.hs = params->hs, hp.vs = params->vs, hp.std_bytes = kStdHeaderBytes[channels == 3];
    for (int c = 0; c < 2; ++c)
        for (int i = 0; i < 64; ++i) {
            qt.q8[c][i] = (uint16_t)(quantiser(c, i, params->quality) << 3);
            hp.q[c][i] = (uint8_t)quantiser(c, kZigzag[i], params->quality);
        }
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    int16_t* coef = (int16_t*)ws;
    uint32_t* len = (uint32_t*)(ws + g.off_len);
    uint32_t* cnt = (uint32_t*)(ws + g.off_cnt);
    uint32_t* tot = (uint32_t*)(ws + g.off_tot);          // [0] bits of the scan, [1] its 0xFF bytes
    JDev* dev = params->optimize ? (JDev*)(ws + g.off_dev) : nullptr;
    uint32_t* bits = (uint32_t*)(ws + g.off_stream);
    uint32_t* hist = dev ? &dev->hist[0][0] : nullptr;
    const unsigned per_block = (g.nblocks + 255) / 256, grid = (g.units + 3) / 4;
    const uint32_t nb = (uint32_t)g.nb, ny = (uint32_t)g.ny;
    if (channels == 1)
        hipLaunchKernelGGL((jpeg_blocks_kernel<1, 1, 1>), dim3(grid), dim3(256), 0, st, (const uint8_t*)src, coef, g, qt, hist);
    else if (params->hs == 1)
        hipLaunchKernelGGL((jpeg_blocks_kernel<3, 1, 1>), dim3(grid), dim3(256), 0, st, (const uint8_t*)src, coef, g, qt, hist);
    else if (params->vs == 1)
        hipLaunchKernelGGL((jpeg_blocks_kernel<3, 2, 1>), dim3(grid), dim3(256), 0, st, (const uint8_t*)src, coef, g, qt, hist);
    else
        hipLaunchKernelGGL((jpeg_blocks_kernel<3, 2, 2>), dim3(grid), dim3(256), 0, st, (const uint8_t*)src, coef, g, qt, hist);
    ST_CHECK_LAUNCH();
    const unsigned zero_grid = (g.stream_words + 255) / 256 < 512 ? (g.stream_words + 255) / 256 : 512;
    if (rg.ri) {                                                       // restart intervals: what differs is csrc/jpeg_rst.hip's
        JpegRstEncode e;
        e.coef = coef, e.len = len, e.tot = tot, e.pad = (uint32_t*)(ws + rg.off_pad), e.ibyte = (uint32_t*)(ws + rg.off_ibyte);
        e.stream = bits, e.stream_words = g.stream_words, e.dev = dev;
        e.nblocks = g.nblocks, e.nb = nb, e.ny = ny, e.ri = rg.ri, e.nint = rg.nint, e.nchunks = g.nchunks;
        e.cnt = cnt, e.out = (uint8_t*)out, e.out_nbytes = out_nbytes, e.header = &hp, e.st = st;
        int rc;
        if (dev) {
            if ((rc = st_jpeg_rst_hist(e)) != ST_OK) return rc;
            hipLaunchKernelGGL(jpeg_table_kernel, dim3(channels == 3 ? 4 : 2), dim3(64), 0, st, dev);
            ST_CHECK_LAUNCH();
        }
        if ((rc = st_jpeg_rst_offsets(e)) != ST_OK) return rc;
        hipLaunchKernelGGL(jpeg_zero_kernel, dim3(zero_grid), dim3(256), 0, st, bits, (const uint32_t*)tot, g.stream_words);
        ST_CHECK_LAUNCH();
        if ((rc = st_jpeg_rst_pack(e)) != ST_OK) return rc;
        hipLaunchKernelGGL(jpeg_count_kernel, dim3(g.nchunks), dim3(256), 0, st, (const uint32_t*)bits, (const uint32_t*)tot, cnt);
        ST_CHECK_LAUNCH();
        hipLaunchKernelGGL(jpeg_scan_kernel, dim3(1), dim3(1024), 0, st, cnt, g.nchunks, (const uint32_t*)tot, tot + 1);
        ST_CHECK_LAUNCH();
        return st_jpeg_rst_stuff(e);
    }
    if (dev) {
        hipLaunchKernelGGL(jpeg_hist_kernel, dim3(per_block), dim3(256), 0, st, (const int16_t*)coef, hist, g.nblocks, nb, ny);
        ST_CHECK_LAUNCH();
        hipLaunchKernelGGL(jpeg_table_kernel, dim3(channels == 3 ? 4 : 2), dim3(64), 0, st, dev);
        ST_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(jpeg_bits_kernel, dim3(per_block), dim3(256), 0, st, (const int16_t*)coef, len, (const JDev*)dev, g.nblocks, nb, ny);
    ST_CHECK_LAUNCH();
    hipLaunchKernelGGL(jpeg_scan_kernel, dim3(1), dim3(1024), 0, st, len, g.nblocks, (const uint32_t*)nullptr, tot);
    ST_CHECK_LAUNCH();
    hipLaunchKernelGGL(jpeg_zero_kernel, dim3(zero_grid), dim3(256), 0, st, bits, (const uint32_t*)tot, g.stream_words);
    ST_CHECK_LAUNCH();
    hipLaunchKernelGGL(jpeg_pack_kernel, dim3(per_block), dim3(256), 0, st, (const int16_t*)coef, (const uint32_t*)len, (const uint32_t*)tot, bits, g.stream_words,
                       (const JDev*)dev, g.nblocks, nb, ny);
    ST_CHECK_LAUNCH();
    hipLaunchKernelGGL(jpeg_count_kernel, dim3(g.nchunks), dim3(256), 0, st, (const uint32_t*)bits, (const uint32_t*)tot, cnt);
    ST_CHECK_LAUNCH();
    hipLaunchKernelGGL(jpeg_scan_kernel, dim3(1), dim3(1024), 0, st, cnt, g.nchunks, (const uint32_t*)tot, tot + 1);
    ST_CHECK_LAUNCH();
    hipLaunchKernelGGL(jpeg_stuff_kernel, dim3(g.nchunks), dim3(256), 0, st, (const uint32_t*)bits, (const uint32_t*)tot, (const uint32_t*)cnt, (uint8_t*)out, out_nbytes,
                       hp, (const JDev*)dev);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

extern "C" int st_jpeg_workspace_bytes(int32_t H, int32_t W, int32_t channels) {
    const st_jpeg_enc_params p = default_params(channels);
    return st_jpeg_workspace_bytes_ex(H, W, channels, &p);
}

extern "C" int st_jpeg_max_bytes(int32_t H, int32_t W, int32_t channels) {
    const st_jpeg_enc_params p = default_params(channels);
    return st_jpeg_max_bytes_ex(H, W, channels, &p);
}

extern "C" int st_jpeg_encode_u8(const void* src, int32_t H, int32_t W, int32_t channels, int64_t row_stride, void* out, int64_t out_capacity,
                                 int32_t* out_nbytes, void* workspace, int64_t workspace_bytes, void* stream) {
    const st_jpeg_enc_params p = default_params(channels);
    return st_jpeg_encode_u8_ex(src, H, W, channels, row_stride, &p, out, out_capacity, out_nbytes, workspace, workspace_bytes, stream);
}

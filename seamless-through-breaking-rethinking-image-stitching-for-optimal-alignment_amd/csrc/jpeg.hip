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
//
// With restart intervals (st_jpeg_enc_params.reserved[0] = Ri > 0) the file is the one Pillow's `save(restart_marker_blocks= /
// restart_marker_rows=)` writes, byte for byte.  The block, table, zero, count and scan kernels are the ones above.  The histogram, bits, pack
// and stuff steps are each written once, as a body on `bool RST`; the kernels of both paths are its two instantiations:
//
//   jpegr_enc_hist_kernel     jpeg_hist_kernel with the DC predecessor 0 for a component's first block of an interval (optimize only)
//   jpegr_enc_bits_kernel     jpeg_bits_kernel with the same predecessor rule; jpeg_scan_kernel makes unpadded bit offsets from the lengths
//   jpegr_enc_pad_kernel      one thread per interval: the 1-bits that round its end up to a byte; jpeg_scan_kernel sums them
//   jpegr_enc_offsets_kernel  bit offset of every block in the padded stream, the byte every interval starts at, the padded stream's bits
//   jpegr_enc_pack_kernel     jpeg_pack_kernel with the predecessor rule; an interval's last block appends the padding
//   jpegr_enc_stuff_kernel    jpeg_stuff_kernel: a byte's position adds two for every interval boundary in front of it, the thread that owns an
//                             interval's first byte writes FF D0+((k-1)&7) in front of it, unstuffed; the DRI segment goes in front of SOS
#include "common.h"
#include "jpeg_tables.h"
#include "jpeg_huff_core.h"
#include "jpeg_scan.h"
#include "../../include/stitch_gfx950.h"

namespace {

// ---- code tables, header ----------------------------------------------------------------------------------------------------------
constexpr int kDhtMax = 16 + 256;
struct JTabs {                         // the four tables in DHT order: DC0, AC0, DC1, AC1
    uint32_t code[4][256];             // by symbol (DC: the category): code | length << 16
    uint8_t dht[4][kDhtMax];           // the DHT payload behind the Tc / Th byte: 16 counts, then the symbols
    int32_t dht_len[4];
};

constexpr JTabs make_std() {           // ITU-T T.81 Annex K (csrc/jpeg_tables.h), canonical codes (Annex C)
    JTabs t{};
    for (int c = 0; c < 2; ++c) {
        for (int ac = 0; ac < 2; ++ac) {
            const int* bits = ac ? kAcBits[c] : kDcBits[c];
            const int nsym = ac ? 162 : 12, i = 2 * c + ac;
            uint32_t code = 0;
            int k = 0;
            for (int len = 1; len <= 16; ++len) {
                t.dht[i][len - 1] = (uint8_t)bits[len - 1];
                for (int j = 0; j < bits[len - 1]; ++j, ++k) t.code[i][ac ? kAcVals[c][k] : k] = code++ | ((uint32_t)len << 16);
                code <<= 1;
            }
            for (int j = 0; j < nsym; ++j) t.dht[i][16 + j] = (uint8_t)(ac ? kAcVals[c][j] : j);
            t.dht_len[i] = 16 + nsym;
        }
    }
    return t;
}

struct JIzz {
    uint8_t v[64];                     // natural index -> zigzag position
};
constexpr JIzz make_izz() {
    JIzz z{};
    for (int i = 0; i < 64; ++i) z.v[kZigzag[i]] = (uint8_t)i;
    return z;
}

// SOI + APP0, DQT x n, SOF0, DHT x 2n, SOS: what write_header writes.  (All four lengths are read, needed or not: four loads in flight, where a
// loop over the tables in use would wait for each -- in every workgroup of the stuff kernel.)
constexpr uint32_t header_bytes(int ncomp, const JTabs& tabs) {
    const uint32_t luma = 69u + 2 * 5u + (uint32_t)tabs.dht_len[0] + (uint32_t)tabs.dht_len[1];
    const uint32_t chroma = 69u + 2 * 5u + (uint32_t)tabs.dht_len[2] + (uint32_t)tabs.dht_len[3];
    return 20u + (10u + 3 * ncomp) + (8u + 2 * ncomp) + luma + (ncomp == 3 ? chroma : 0u);
}

constexpr JTabs kStdHost = make_std();
// no table has more symbols than the Annex K ones, so no header is longer than theirs
constexpr uint32_t kStdHeaderBytes[2] = {header_bytes(1, kStdHost), header_bytes(3, kStdHost)};
static_assert(kStdHeaderBytes[0] == 328 && kStdHeaderBytes[1] == 623, "header sizes of the contract");
__device__ const JTabs g_std = make_std();

struct JDev {                          // the workspace's table area (optimize only)
    JTabs tabs;
    uint32_t hist[4][kJhEntries];
};

struct JHeader {
    int32_t H, W, ncomp, hs, vs;
    uint32_t std_bytes;                // the header's length with the Annex K tables: the plain path starts without a read for it
    uint8_t q[2][64];                  // zigzag order, as DQT lists them
};

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

// restart intervals (reserved[0] = Ri MCUs > 0): n = ceil(MCUs / Ri) intervals.  Each adds at most 7 padding bits to the
// stream (counted as a byte, doubled like every byte for stuffing: 2 bytes of the file) and one two-byte marker; the DRI segment is 6 bytes.
// The workspace grows by the stream's share of that and by two tables of n + 1 words behind the stream.  (Kept beside JGeom and not in it:
// JGeom is an argument of jpeg_blocks_kernel, which has no use for them.)
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
struct HuffLds {
    uint32_t dc[2][16];
    uint32_t ac[2][256];
};

__device__ __forceinline__ void load_huff(HuffLds& h, const JTabs* __restrict__ tabs) {
    for (int i = threadIdx.x; i < 512; i += blockDim.x) h.ac[i >> 8][i & 255] = tabs->code[2 * (i >> 8) + 1][i & 255];
    if (threadIdx.x < 32) h.dc[threadIdx.x >> 4][threadIdx.x & 15] = tabs->code[2 * (threadIdx.x >> 4)][threadIdx.x & 15];
    __syncthreads();
}

// scan-order predecessor of block b inside its component (-1: none) and the block's table (0 luma, 1 chroma)
__device__ __forceinline__ int64_t block_pred(uint32_t b, uint32_t nb, uint32_t ny, int& table) {
    table = 0;
    if (nb == 1) return (int64_t)b - 1;
    const uint32_t m = b / nb, j = b - m * nb;
    table = j >= ny;
    if (j >= 1 && j < ny) return (int64_t)b - 1;
    if (m == 0) return -1;
    return (int64_t)(m - 1) * nb + (j == 0 ? ny - 1 : j);
}

// the DC value block b is predicted from: its scan-order predecessor in the component, 0 at the start of the scan and (RST) of an interval
template <bool RST>
__device__ __forceinline__ int dc_pred(const int16_t* __restrict__ coef, uint32_t b, uint32_t nb, uint32_t ny, uint32_t ri, int& table) {
    const int64_t pb = block_pred(b, nb, ny, table);
    if constexpr (RST) {
        if (pb < 0 || ((uint32_t)pb / nb) / ri != (b / nb) / ri) return 0;
        return (int)coef[pb * 64];
    } else {
        return pb < 0 ? 0 : (int)coef[pb * 64];
    }
}

__device__ __forceinline__ int coef_at(const uint4& w, int e) {      // e: constant after unrolling
    const uint32_t d = e < 2 ? w.x : e < 4 ? w.y : e < 6 ? w.z : w.w;
    return (int)(int16_t)((e & 1) ? (d >> 16) : (d & 0xffffu));
}

__device__ __forceinline__ int magnitude_bits(int v) { return 32 - __clz(abs(v)); }

// the symbols of block b in scan order: dc(category, difference), then per nonzero coefficient zrl(k), the k >= 0 ZRL symbols (0xF0) of a run
// above 15, and ac(run << 4 | size, value, size) with the rest of the run; EOB is ac(0x00, 0, 0)
template <class DC, class ZRL, class AC>
__device__ __forceinline__ void walk_block(const int16_t* __restrict__ coef, uint32_t b, int pred, DC&& dc, ZRL&& zrl, AC&& ac) {
    const uint4* c4 = (const uint4*)(coef + (size_t)b * 64);
    int run = 0;
#pragma unroll 1
    for (int q = 0; q < 8; ++q) {
        const uint4 w = c4[q];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int v = coef_at(w, e);
            if (q == 0 && e == 0) {
                dc(magnitude_bits(v - pred), v - pred);
            } else if (v == 0) {
                ++run;
            } else {
                zrl(run >> 4);
                const int n = magnitude_bits(v);
                ac(((run & 15) << 4) | n, v, n);
                run = 0;
            }
        }
    }
    if (run) ac(0x00, 0, 0);
}

// The histogram, bits, pack and stuff steps follow, each as one body for a plain file (RST false) and a file with restart intervals of
// `ri` MCUs (RST true); what the other path's kernel has no argument for is passed as 0 / nullptr and never read.
template <bool RST>
__device__ __forceinline__ void hist_body(const int16_t* __restrict__ coef, uint32_t* __restrict__ hist, uint32_t nblocks, uint32_t nb, uint32_t ny, uint32_t ri) {
    __shared__ uint32_t s_hist[4 * kJhEntries];
    for (int i = threadIdx.x; i < 4 * kJhEntries; i += 256) s_hist[i] = 0u;
    __syncthreads();
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b < nblocks) {
        int t;
        const int pred = dc_pred<RST>(coef, b, nb, ny, ri, t);
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

__global__ __launch_bounds__(256) void jpeg_hist_kernel(const int16_t* __restrict__ coef, uint32_t* __restrict__ hist, uint32_t nblocks, uint32_t nb, uint32_t ny) {
    hist_body<false>(coef, hist, nblocks, nb, ny, 0u);
}

__global__ __launch_bounds__(256) void jpegr_enc_hist_kernel(const int16_t* __restrict__ coef, uint32_t* __restrict__ hist, uint32_t nblocks, uint32_t nb, uint32_t ny,
                                                             uint32_t ri) {
    hist_body<true>(coef, hist, nblocks, nb, ny, ri);
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
template <bool RST>
__device__ __forceinline__ void bits_body(const int16_t* __restrict__ coef, uint32_t* __restrict__ len, const JDev* __restrict__ dev, uint32_t nblocks, uint32_t nb,
                                          uint32_t ny, uint32_t ri) {
    __shared__ HuffLds h;
    load_huff(h, dev ? &dev->tabs : &g_std);
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nblocks) return;
    int t;
    const int pred = dc_pred<RST>(coef, b, nb, ny, ri, t);
    uint32_t bits = 0;
    walk_block(
        coef, b, pred, [&](int n, int) { bits += (h.dc[t][n & 15] >> 16) + n; }, [&](int k) { bits += (uint32_t)k * (h.ac[t][0xF0] >> 16); },
        [&](int sym, int, int n) { bits += (h.ac[t][sym & 255] >> 16) + n; });
    len[b] = bits;
}

__global__ __launch_bounds__(256) void jpeg_bits_kernel(const int16_t* __restrict__ coef, uint32_t* __restrict__ len, const JDev* __restrict__ dev, uint32_t nblocks,
                                                        uint32_t nb, uint32_t ny) {
    bits_body<false>(coef, len, dev, nblocks, nb, ny, 0u);
}

__global__ __launch_bounds__(256) void jpegr_enc_bits_kernel(const int16_t* __restrict__ coef, uint32_t* __restrict__ len, const JDev* __restrict__ dev, uint32_t nblocks,
                                                             uint32_t nb, uint32_t ny, uint32_t ri) {
    bits_body<true>(coef, len, dev, nblocks, nb, ny, ri);
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

// off: the exclusive prefix sum of the blocks' bits, tot[0] their sum.  Every interval starts on a byte, so its padding is its own bits' alone.
__global__ __launch_bounds__(256) void jpegr_enc_pad_kernel(const uint32_t* __restrict__ off, const uint32_t* __restrict__ tot, uint32_t* __restrict__ pad, uint32_t nblocks,
                                                            uint32_t per, uint32_t nint) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nint) return;
    const uint32_t s = i * per, e = s + per;                            // per = Ri * blocks per MCU <= 6 * 65535
    const uint32_t bits = (e < nblocks ? off[e] : tot[0]) - off[s];
    pad[i] = (8u - (bits & 7u)) & 7u;
}

// pad: the exclusive prefix sum of the padding bits, tot[2] their sum
__global__ __launch_bounds__(256) void jpegr_enc_offsets_kernel(uint32_t* __restrict__ off, uint32_t* __restrict__ tot, const uint32_t* __restrict__ pad,
                                                                uint32_t* __restrict__ ibyte, uint32_t nblocks, uint32_t per) {
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nblocks) return;
    const uint32_t i = b / per, o = off[b] + pad[i];
    off[b] = o;
    if (b == i * per) ibyte[i] = o >> 3;
    if (b == 0) tot[0] += tot[2];                                       // (read by no other thread of this launch)
}

struct BitWriter {
    uint32_t* word;      // next word of the stream (bytes in stream order: the big-endian word, byte-swapped)
    uint32_t* end;       // one past the stream's capacity: nothing is written from here on
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
        if (w.word < w.end) {
            if (w.first) atomicOr(w.word, word);
            else *w.word = word;
        }
        w.first = false;
        ++w.word;
    }
}

template <bool RST>
__device__ __forceinline__ void pack_body(const int16_t* __restrict__ coef, const uint32_t* __restrict__ off, const uint32_t* __restrict__ total_bits,
                                          uint32_t* __restrict__ stream, uint32_t cap_words, const JDev* __restrict__ dev, uint32_t nblocks, uint32_t nb, uint32_t ny,
                                          uint32_t ri) {
    __shared__ HuffLds h;
    load_huff(h, dev ? &dev->tabs : &g_std);
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nblocks) return;
    int t;
    const int pred = dc_pred<RST>(coef, b, nb, ny, ri, t);
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
    if constexpr (RST) {
        if (b + 1 == nblocks || (b + 1) % (ri * nb) == 0) {             // the interval's final partial byte is padded with 1-bits (words are byte multiples)
            const int pad = (8 - (w.n & 7)) & 7;
            put_bits(w, (1u << pad) - 1u, pad);
        }
    } else {
        if (b == nblocks - 1) {                                       // the final partial byte is padded with 1-bits
            const int pad = (int)((8u - (*total_bits & 7u)) & 7u);
            put_bits(w, (1u << pad) - 1u, pad);
        }
    }
    if (w.n > 0 && w.word < w.end) atomicOr(w.word, __builtin_bswap32((uint32_t)(w.acc << (32 - w.n))));
}

__global__ __launch_bounds__(256) void jpeg_pack_kernel(const int16_t* __restrict__ coef, const uint32_t* __restrict__ off, const uint32_t* __restrict__ total_bits,
                                                        uint32_t* __restrict__ stream, uint32_t cap_words, const JDev* __restrict__ dev, uint32_t nblocks, uint32_t nb,
                                                        uint32_t ny) {
    pack_body<false>(coef, off, total_bits, stream, cap_words, dev, nblocks, nb, ny, 0u);
}

__global__ __launch_bounds__(256) void jpegr_enc_pack_kernel(const int16_t* __restrict__ coef, const uint32_t* __restrict__ off, uint32_t* __restrict__ stream,
                                                             uint32_t cap_words, const JDev* __restrict__ dev, uint32_t nblocks, uint32_t nb, uint32_t ny, uint32_t ri) {
    pack_body<true>(coef, off, nullptr, stream, cap_words, dev, nblocks, nb, ny, ri);
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

// SOI, APP0, DQT x n, SOF0, DHT x n (DC0, AC0, DC1, AC1), SOS; one workgroup
__device__ __forceinline__ void write_header(uint8_t* __restrict__ out, const JHeader& hp, const JTabs* __restrict__ tabs) {
    const int ntab = hp.ncomp == 3 ? 2 : 1, nc = hp.ncomp, tid = threadIdx.x;
    uint32_t n = 0;
    if (tid < 20) {
        const uint32_t lo = 0xE0FFD8FFu, mid = 0x464A1000u;                      // FF D8 FF E0 | 00 10 'J' 'F'
        const uint8_t rest[12] = {'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
        uint8_t v = 0;
        if (tid < 4) v = (uint8_t)(lo >> (8 * tid));
        else if (tid < 8) v = (uint8_t)(mid >> (8 * (tid - 4)));
#pragma unroll
        for (int k = 0; k < 12; ++k)
            if (tid == 8 + k) v = rest[k];
        out[tid] = v;
    }
    n = 20;
    for (int c = 0; c < ntab; ++c, n += 69) {
        if (tid < 5) out[n + tid] = tid == 0 ? 0xFF : tid == 1 ? 0xDB : tid == 2 ? 0 : tid == 3 ? 67 : (uint8_t)c;
        if (tid < 64) out[n + 5 + tid] = hp.q[c][tid];
    }
    if (tid == 0) {
        uint8_t* h = out + n;
        h[0] = 0xFF, h[1] = 0xC0, h[2] = 0, h[3] = (uint8_t)(8 + 3 * nc), h[4] = 8;
        h[5] = (uint8_t)(hp.H >> 8), h[6] = (uint8_t)(hp.H & 255), h[7] = (uint8_t)(hp.W >> 8), h[8] = (uint8_t)(hp.W & 255), h[9] = (uint8_t)nc;
        for (int c = 0; c < nc; ++c) h[10 + 3 * c] = (uint8_t)(c + 1), h[11 + 3 * c] = c ? 0x11 : (uint8_t)(hp.hs << 4 | hp.vs), h[12 + 3 * c] = c ? 1 : 0;
    }
    n += 10 + 3 * nc;
    for (int i = 0; i < 2 * ntab; ++i) {
        const uint32_t len = (uint32_t)tabs->dht_len[i];
        if (tid < 5) out[n + tid] = tid == 0 ? 0xFF : tid == 1 ? 0xC4 : tid == 2 ? (uint8_t)((len + 3) >> 8) : tid == 3 ? (uint8_t)((len + 3) & 255) : (uint8_t)((i & 1) << 4 | (i >> 1));
        for (uint32_t k = tid; k < len; k += 256) out[n + 5 + k] = tabs->dht[i][k];
        n += 5 + len;
    }
    if (tid == 0) {
        uint8_t* h = out + n;
        h[0] = 0xFF, h[1] = 0xDA, h[2] = 0, h[3] = (uint8_t)(6 + 2 * nc), h[4] = (uint8_t)nc;
        for (int c = 0; c < nc; ++c) h[5 + 2 * c] = (uint8_t)(c + 1), h[6 + 2 * c] = c ? 0x11 : 0x00;
        h[5 + 2 * nc] = 0, h[6 + 2 * nc] = 63, h[7 + 2 * nc] = 0;
    }
}

// RST: ibyte[1 .. nint - 1], the stream byte every interval starts at, is strictly increasing (an interval holds at least one block, a block at
// least two bits, and ends on a byte)
template <bool RST>
__device__ __forceinline__ void stuff_body(const uint32_t* __restrict__ stream, const uint32_t* __restrict__ totals, const uint32_t* __restrict__ cnt_off,
                                           const uint32_t* __restrict__ ibyte, uint32_t nint, uint32_t ri, uint8_t* __restrict__ out, int32_t* __restrict__ out_nbytes,
                                           const JHeader& hp, const JDev* __restrict__ dev) {
    __shared__ uint32_t s_wave[4];
    const JTabs* tabs = dev ? &dev->tabs : &g_std;
    const uint32_t nbytes = (totals[0] + 7u) >> 3;
    const uint32_t hdr0 = dev ? header_bytes(hp.ncomp, dev->tabs) : hp.std_bytes, hdr = RST ? hdr0 + 6u : hdr0;
    // the header is the last workgroup's: its chunk lies behind the stream unless the image fills the worst case, so the header is written
    // beside the scatter and not in front of workgroup 0's
    if (blockIdx.x == gridDim.x - 1) {
        write_header(out, hp, tabs);
        if (threadIdx.x == 0) {
            if constexpr (RST) {                                        // (this thread wrote SOS: it moves six bytes back, DRI takes its place)
                const uint32_t sos = 8u + 2u * (uint32_t)hp.ncomp;
                uint8_t* h = out + hdr0 - sos;
                for (int k = (int)sos - 1; k >= 0; --k) h[k + 6] = h[k];
                h[0] = 0xFF, h[1] = 0xDD, h[2] = 0, h[3] = 4, h[4] = (uint8_t)(ri >> 8), h[5] = (uint8_t)(ri & 255u);
            }
            const uint32_t end = hdr + nbytes + totals[1] + (RST ? 2u * (nint - 1u) : 0u);      // a marker in front of every interval but the first
            out[end] = 0xFF, out[end + 1] = 0xD9;
            *out_nbytes = (int32_t)(end + 2);
        }
    }
    if (blockIdx.x * kChunk >= nbytes) return;
    const uint32_t i0 = blockIdx.x * kChunk + threadIdx.x * 8;
    const uint2 d = i0 < nbytes ? *(const uint2*)(stream + (i0 >> 2)) : make_uint2(0u, 0u);
    uint32_t ex;
    block_sum_256(ff_bytes(d, i0, nbytes), ex, s_wave);
    uint32_t m = 0;                                                     // RST: the intervals 1 .. nint - 1 that start in front of byte i0
    if constexpr (RST) {
        uint32_t lo = 0, hi = nint;
        while (hi - lo > 1u) {                                          // ibyte[lo] < i0 or lo == 0; ibyte[hi] >= i0 or hi == nint
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (ibyte[mid] < i0) lo = mid;
            else hi = mid;
        }
        m = lo;
    }
    uint8_t* o = out + hdr + i0 + cnt_off[blockIdx.x] + ex + 2u * m;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t byte = ((k < 4 ? d.x : d.y) >> ((k & 3) * 8)) & 255u;
        if (i0 + k < nbytes) {
            if constexpr (RST) {
                if (m + 1u < nint && ibyte[m + 1u] == i0 + k) {
                    *o++ = 0xFF, *o++ = (uint8_t)(0xD0u + (m & 7u));
                    ++m;
                }
            }
            *o++ = (uint8_t)byte;
            if (byte == 255u) *o++ = 0;
        }
    }
}

__global__ __launch_bounds__(256) void jpeg_stuff_kernel(const uint32_t* __restrict__ stream, const uint32_t* __restrict__ totals, const uint32_t* __restrict__ cnt_off,
                                                         uint8_t* __restrict__ out, int32_t* __restrict__ out_nbytes, const JHeader hp, const JDev* __restrict__ dev) {
    stuff_body<false>(stream, totals, cnt_off, nullptr, 0u, 0u, out, out_nbytes, hp, dev);
}

__global__ __launch_bounds__(256) void jpegr_enc_stuff_kernel(const uint32_t* __restrict__ stream, const uint32_t* __restrict__ totals, const uint32_t* __restrict__ cnt_off,
                                                              const uint32_t* __restrict__ ibyte, uint32_t nint, uint32_t ri, uint8_t* __restrict__ out,
                                                              int32_t* __restrict__ out_nbytes, const JHeader hp, const JDev* __restrict__ dev) {
    stuff_body<true>(stream, totals, cnt_off, ibyte, nint, ri, out, out_nbytes, hp, dev);
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
    // restart intervals (ri > 0): the kernels of the RST instantiations, and between the bits and the zero step the padding of every interval
    const uint32_t ri = rg.ri, per = ri * nb;
    uint32_t* pad = (uint32_t*)(ws + rg.off_pad);          // [nint + 1]: padding bits behind interval i, then their exclusive prefix sum
    uint32_t* ibyte = (uint32_t*)(ws + rg.off_ibyte);      // [nint + 1]: the stream byte interval i starts at
    if (dev) {
        if (ri) hipLaunchKernelGGL(jpegr_enc_hist_kernel, dim3(per_block), dim3(256), 0, st, (const int16_t*)coef, hist, g.nblocks, nb, ny, ri);
        else hipLaunchKernelGGL(jpeg_hist_kernel, dim3(per_block), dim3(256), 0, st, (const int16_t*)coef, hist, g.nblocks, nb, ny);
        ST_CHECK_LAUNCH();
        hipLaunchKernelGGL(jpeg_table_kernel, dim3(channels == 3 ? 4 : 2), dim3(64), 0, st, dev);
        ST_CHECK_LAUNCH();
    }
    if (ri) hipLaunchKernelGGL(jpegr_enc_bits_kernel, dim3(per_block), dim3(256), 0, st, (const int16_t*)coef, len, (const JDev*)dev, g.nblocks, nb, ny, ri);
    else hipLaunchKernelGGL(jpeg_bits_kernel, dim3(per_block), dim3(256), 0, st, (const int16_t*)coef, len, (const JDev*)dev, g.nblocks, nb, ny);
    ST_CHECK_LAUNCH();
    hipLaunchKernelGGL(jpeg_scan_kernel, dim3(1), dim3(1024), 0, st, len, g.nblocks, (const uint32_t*)nullptr, tot);
    ST_CHECK_LAUNCH();
    if (ri) {                                              // tot[2]: padding bits; tot[0] becomes the bits of the padded stream
        hipLaunchKernelGGL(jpegr_enc_pad_kernel, dim3((rg.nint + 255) / 256), dim3(256), 0, st, (const uint32_t*)len, (const uint32_t*)tot, pad, g.nblocks, per, rg.nint);
        ST_CHECK_LAUNCH();
        hipLaunchKernelGGL(jpeg_scan_kernel, dim3(1), dim3(1024), 0, st, pad, rg.nint, (const uint32_t*)nullptr, tot + 2);
        ST_CHECK_LAUNCH();
        hipLaunchKernelGGL(jpegr_enc_offsets_kernel, dim3(per_block), dim3(256), 0, st, len, tot, (const uint32_t*)pad, ibyte, g.nblocks, per);
        ST_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(jpeg_zero_kernel, dim3(zero_grid), dim3(256), 0, st, bits, (const uint32_t*)tot, g.stream_words);
    ST_CHECK_LAUNCH();
    if (ri)
        hipLaunchKernelGGL(jpegr_enc_pack_kernel, dim3(per_block), dim3(256), 0, st, (const int16_t*)coef, (const uint32_t*)len, bits, g.stream_words, (const JDev*)dev,
                           g.nblocks, nb, ny, ri);
    else
        hipLaunchKernelGGL(jpeg_pack_kernel, dim3(per_block), dim3(256), 0, st, (const int16_t*)coef, (const uint32_t*)len, (const uint32_t*)tot, bits, g.stream_words,
                           (const JDev*)dev, g.nblocks, nb, ny);
    ST_CHECK_LAUNCH();
    hipLaunchKernelGGL(jpeg_count_kernel, dim3(g.nchunks), dim3(256), 0, st, (const uint32_t*)bits, (const uint32_t*)tot, cnt);
    ST_CHECK_LAUNCH();
    hipLaunchKernelGGL(jpeg_scan_kernel, dim3(1), dim3(1024), 0, st, cnt, g.nchunks, (const uint32_t*)tot, tot + 1);
    ST_CHECK_LAUNCH();
    if (ri)
        hipLaunchKernelGGL(jpegr_enc_stuff_kernel, dim3(g.nchunks), dim3(256), 0, st, (const uint32_t*)bits, (const uint32_t*)tot, (const uint32_t*)cnt, (const uint32_t*)ibyte,
                           rg.nint, ri, (uint8_t*)out, out_nbytes, hp, (const JDev*)dev);
    else
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

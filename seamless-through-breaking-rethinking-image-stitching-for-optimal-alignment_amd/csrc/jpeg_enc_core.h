// What the JPEG encoder's translation units (csrc/jpeg.hip, and csrc/jpeg_rst.hip for files with restart intervals) share: the code tables,
// the header, the walk over a block's symbols and the bit writer.  Everything has internal linkage.
#pragma once
#include "common.h"
#include "jpeg_tables.h"
#include "jpeg_huff_core.h"

namespace {

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

__device__ __forceinline__ uint32_t ff_bytes(uint2 d, uint32_t i0, uint32_t nbytes) {
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t byte = ((k < 4 ? d.x : d.y) >> ((k & 3) * 8)) & 255u;
        c += (i0 + k < nbytes && byte == 255u) ? 1u : 0u;
    }
    return c;
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

}  // namespace

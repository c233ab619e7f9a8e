// Entropy decoding of a baseline JPEG scan with restart intervals (DRI > 0), the part of st_jpeg_decode_u8 between the file's bytes and the
// DC-predicted coefficients (contract: README.md "Restart intervals"; CPU restatement: tests/_jpeg_rst_ref.py; the cutting rules in plain
// C++: csrc/jpeg_rst_core.h).  An interval starts byte-aligned behind a marker that cannot occur in the data, with DC predictions 0 and at
// a known MCU: no decoder state is guessed at its start and nothing crosses from one interval to the next.  Integer arithmetic only.
//
//   jpegr_count_kernel    per 2048-byte chunk of the scan: the bytes that are not part of the stream (a 0x00 behind a 0xFF, both bytes of a
//                         restart marker) and the restart markers; jpeg_scan_kernel (csrc/jpeg.hip) scans both
//   jpegr_unstuff_kernel  compacts the scan to the unstuffed stream without its markers, 16 zero bytes behind it; writes the stream offset
//                         behind every marker
//   jpegr_cut_kernel      one thread per interval: its start in the stream and its number of 1024-bit subsequences; jpeg_scan_kernel makes
//                         the first subsequence of every interval from them.  Clears the status word
//   jpegr_sync_kernel     one thread per subsequence: an interval's first subsequence decodes from its known state, the others from a guess
//                         (their first bit, slot 0, DC next); the workgroup repeats `start[j] <- end[j - 1]` inside every interval to its
//                         fixpoint.  Launched once per workgroup of subsequences as in csrc/jpeg_dec.hip: launch r carries the states over r
//                         workgroup boundaries and returns at once when the launch before it moved no workgroup's end state
//   jpeg_scan_kernel      blocks completed per subsequence -> blocks in front of every subsequence
//   jpegr_write_kernel    decodes every subsequence again from its final state and writes the coefficients into its interval's blocks only;
//                         an interval whose bytes held another number of blocks than it has sets bit 0 (fewer) or bit 1 (more) of the status
//   jpegr_dc_kernel       one workgroup per component: prefix sum of the DC differences that restarts at every interval
//
// And the encoder's side (st_jpeg_encode_u8_ex with st_jpeg_enc_params.reserved[0] = Ri > 0; csrc/jpeg.hip keeps the block, table, zero, count
// and scan kernels): the file Pillow's `save(restart_marker_blocks= / restart_marker_rows=)` writes, byte for byte.
//
//   jpegr_enc_hist_kernel     jpeg_hist_kernel with the DC predecessor 0 for a component's first block of an interval (optimize only)
//   jpegr_enc_bits_kernel     jpeg_bits_kernel with the same predecessor rule; jpeg_scan_kernel makes unpadded bit offsets from the lengths
//   jpegr_enc_pad_kernel      one thread per interval: the 1-bits that round its end up to a byte; jpeg_scan_kernel sums them
//   jpegr_enc_offsets_kernel  bit offset of every block in the padded stream, the byte every interval starts at, the padded stream's bits
//   jpegr_enc_pack_kernel     jpeg_pack_kernel with the predecessor rule; an interval's last block appends the padding
//   jpegr_enc_stuff_kernel    jpeg_stuff_kernel: a byte's position adds two for every interval boundary in front of it, the thread that owns an
//                             interval's first byte writes FF D0+((k-1)&7) in front of it, unstuffed; the DRI segment goes in front of SOS
#include "jpeg_rst.h"
#include "jpeg_rst_core.h"
#include "jpeg_scan.h"
#include "jpeg_tables.h"
#include "jpeg_enc_core.h"

namespace {

struct NatTable {
    uint8_t v[64];
};
constexpr NatTable make_nat() {
    NatTable t{};
    for (int i = 0; i < 64; ++i) t.v[i] = (uint8_t)kZigzag[i];
    return t;
}
__device__ const NatTable g_nat = make_nat();

constexpr uint32_t kChunk = 2048;                        // scan bytes per workgroup of the unstuffing passes (256 threads x 8 bytes)
constexpr uint32_t kSyncThreads = 256;                   // subsequences per workgroup
constexpr uint32_t kPad = 16;                            // zero bytes behind the unstuffed stream

inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

struct RGeom {
    uint32_t nint, nchunks, cap, nwg;
    size_t off_drop, off_nmark, off_mark, off_start, off_first, off_state, off_blk, off_bnd, off_flags, bytes;
};

RGeom make_geom(uint32_t scan_len, uint32_t nmcu, uint32_t ri) {
    RGeom g;
    g.nint = (nmcu + ri - 1) / ri;
    g.nchunks = (scan_len + kChunk - 1) / kChunk;
    // an interval of b bytes has max(1, ceil(8 b / 1024)) <= 8 b / 1024 + 1 subsequences
    const uint32_t nsub = (uint32_t)(((uint64_t)scan_len * 8 + kJrSubBits - 1) / kJrSubBits) + g.nint;
    g.nwg = (nsub + kSyncThreads - 1) / kSyncThreads;
    g.cap = g.nwg * kSyncThreads;
    size_t o = 16;                                       // totals: [0] bytes dropped from the scan, [1] markers found
    g.off_drop = o, o += align16((size_t)g.nchunks * 4);
    g.off_nmark = o, o += align16((size_t)g.nchunks * 4);
    g.off_mark = o, o += align16((size_t)(g.nint + 1) * 4);
    g.off_start = o, o += align16((size_t)(g.nint + 1) * 4);
    g.off_first = o, o += align16((size_t)(g.nint + 1) * 4);
    g.off_state = o, o += 4 * align16((size_t)g.cap * 4);               // start pos, start slot | k, end pos, end slot | k
    g.off_blk = o, o += align16((size_t)(g.cap + 1) * 4);               // blocks completed; behind the scan: blocks in front, [cap] all
    g.off_bnd = o, o += align16((size_t)g.nwg * 2 * 2 * 4);
    g.off_flags = o, o += align16((size_t)(g.nwg + 1) * 4);
    g.bytes = o;
    return g;
}

// ---- unstuffing -----------------------------------------------------------------------------------------------------------------
// the 8 scan bytes from i0, the byte before and the byte behind them; bit k of `drop`: byte i0 + k is not part of the stream (a stuffed
// 0x00, or the 0xFF or the 0xD0..0xD7 of a restart marker); bit k of `mark`: it is the second byte of a restart marker
__device__ __forceinline__ void rst_masks(const uint8_t* __restrict__ scan, uint32_t i0, uint32_t n, uint8_t (&b)[8], uint32_t& drop, uint32_t& mark) {
    uint32_t prev = (i0 > 0 && i0 <= n) ? scan[i0 - 1] : 0u;
    const uint32_t behind = (i0 + 8 < n) ? scan[i0 + 8] : 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) b[k] = i0 + k < n ? scan[i0 + k] : (uint8_t)1;
    drop = 0, mark = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t next = k < 7 ? (uint32_t)b[(k + 1) & 7] : behind;
        if (i0 + k < n) {
            const uint32_t c = jr_byte_class(prev, b[k], next);
            drop |= (c & 1u) << k, mark |= (c >> 1) << k;
        }
        prev = b[k];
    }
}

__global__ __launch_bounds__(256) void jpegr_count_kernel(const uint8_t* __restrict__ scan, uint32_t n, uint32_t* __restrict__ ndrop, uint32_t* __restrict__ nmark) {
    __shared__ uint32_t s_a[4], s_b[4];
    uint8_t b[8];
    uint32_t drop, mark, ex;
    rst_masks(scan, blockIdx.x * kChunk + threadIdx.x * 8, n, b, drop, mark);
    const uint32_t d = block_sum_256(__popc(drop), ex, s_a), m = block_sum_256(__popc(mark), ex, s_b);
    if (threadIdx.x == 0) ndrop[blockIdx.x] = d, nmark[blockIdx.x] = m;
}

// mark[i], i = 1 .. nint - 1: the stream offset behind the i-th marker (a marker past the last interval's is dropped and forgotten)
__global__ __launch_bounds__(256) void jpegr_unstuff_kernel(const uint8_t* __restrict__ scan, uint32_t n, const uint32_t* __restrict__ drop_off,
                                                            const uint32_t* __restrict__ mark_off, const uint32_t* __restrict__ tot, uint8_t* __restrict__ dst,
                                                            uint32_t* __restrict__ mark_pos, uint32_t nint) {
    __shared__ uint32_t s_a[4], s_b[4];
    uint8_t b[8];
    const uint32_t i0 = blockIdx.x * kChunk + threadIdx.x * 8;
    uint32_t drop, mark, ex_d, ex_m;
    rst_masks(scan, i0, n, b, drop, mark);
    block_sum_256(__popc(drop), ex_d, s_a);
    block_sum_256(__popc(mark), ex_m, s_b);
    if (i0 < n) {
        uint32_t o = i0 - drop_off[blockIdx.x] - ex_d;                  // kept bytes in front of byte i0: never more than i0
        uint32_t m = mark_off[blockIdx.x] + ex_m + 1;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (i0 + k < n && !((drop >> k) & 1u)) dst[o++] = b[k];
            if ((mark >> k) & 1u) {
                if (m < nint) mark_pos[m] = o;
                ++m;
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < kPad) dst[n - tot[0] + threadIdx.x] = 0;
}

// ---- intervals ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void jpegr_cut_kernel(const uint32_t* __restrict__ mark_pos, const uint32_t* __restrict__ tot, uint32_t scan_len, uint32_t nint,
                                                        uint32_t* __restrict__ start, uint32_t* __restrict__ nsub, int32_t* __restrict__ status) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const uint32_t bytes = scan_len - tot[0], found = tot[1];
    if (i == 0) *status = 0, start[nint] = bytes;
    if (i >= nint) return;
    const uint32_t s0 = jr_start(mark_pos, i, found, bytes), s1 = i + 1 < nint ? jr_start(mark_pos, i + 1, found, bytes) : bytes;
    start[i] = s0;
    nsub[i] = jr_nsub(s1 - s0);
}

// ---- entropy decoding -----------------------------------------------------------------------------------------------------------
struct RScanArgs {
    const uint8_t* file;
    uint32_t nbytes;
    uint32_t dc_off[2], ac_off[2];
    uint32_t nb, ny, td_bits, ta_bits;
    uint32_t nmcu, ri, nint;
};

constexpr uint32_t kDhtBytes = 16 + 256;       // a DHT payload: the code counts, then at most 256 values

// as in csrc/jpeg_dec.hip: the four DHT payloads come into LDS with one coalesced pass (bytes past the end of the file read as 0), four
// threads build the decode tables from there
__device__ __forceinline__ void load_tables(JdTables& t, uint8_t (&raw)[4][kDhtBytes], const RScanArgs& a) {
    for (uint32_t i = threadIdx.x; i < 4 * kDhtBytes; i += blockDim.x) {
        const uint32_t tab = i / kDhtBytes, j = i - tab * kDhtBytes;
        const uint32_t off = tab == 0 ? a.dc_off[0] : tab == 1 ? a.dc_off[1] : tab == 2 ? a.ac_off[0] : a.ac_off[1];     // constant indices
        raw[tab][j] = (off < a.nbytes && j < a.nbytes - off) ? a.file[off + j] : (uint8_t)0;
    }
    __syncthreads();
    if (threadIdx.x < 4) jd_build_huff(threadIdx.x < 2 ? t.dc[threadIdx.x] : t.ac[threadIdx.x - 2], raw[threadIdx.x], kDhtBytes, 0u);
    __syncthreads();
}

constexpr uint32_t kWgWords = kSyncThreads * kJrSubBits / 32;    // stream words a workgroup's subsequences cover at most
constexpr uint32_t kWgLds = kWgWords + 4;                        // + the word its first bit starts in + the two words a symbol that starts in the last bit reaches into

// The subsequences of a workgroup are consecutive pieces of the stream of at most 1024 bits each: from the first one's first bit (a byte
// boundary, inside word `base`) they cover at most 256 * 1024 bits, and a thread reads up to 64 bits past its last own bit.  That part of
// the stream comes into LDS with one coalesced pass; words past the stream's buffer read as 0.
struct WgStream {
    JrSub sub;
    bool live;
    JdScan sc;
};

__device__ __forceinline__ WgStream make_scan(const RScanArgs& a, const uint32_t* __restrict__ words, uint32_t stream_words, uint32_t (&lds)[kWgLds], uint32_t& s_base,
                                              const uint32_t* __restrict__ start, const uint32_t* __restrict__ first, uint32_t j) {
    WgStream w;
    w.live = j < first[a.nint];
    if (w.live) w.sub = jr_sub(start, first, a.nint, a.ri, a.nb, a.nmcu, j);
    else w.sub = JrSub{0, 0, 0, 0, 0, 0, 0};
    if (threadIdx.x == 0) s_base = w.sub.lo >> 5;
    __syncthreads();
    const uint32_t base = s_base;
    for (uint32_t k = threadIdx.x; k < kWgLds; k += blockDim.x) lds[k] = base + k < stream_words ? words[base + k] : 0u;
    __syncthreads();
    w.sc.words = lds, w.sc.base_word = base;
    w.sc.nbits = w.sub.end;
    w.sc.nb = a.nb, w.sc.ny = a.ny;
    w.sc.td_bits = a.td_bits, w.sc.ta_bits = a.ta_bits;
    return w;
}

// state arrays: [4][cap] -- start pos, start (slot << 8 | k), end pos, end (slot << 8 | k); blk[cap]: blocks completed
// bnd: [2][nwg][2] the end state of every workgroup's last subsequence, written by launch r into half r & 1
// flags: [nwg + 1], flags[r] != 0: launch r changed the end state of a workgroup's last subsequence, which is all that launch r + 1 takes
// from it (a start that moved inside a workgroup and synchronised again before its end needs no further launch)
__global__ __launch_bounds__(256) void jpegr_sync_kernel(const RScanArgs a, const uint32_t* __restrict__ words, uint32_t stream_words,
                                                         const uint32_t* __restrict__ start, const uint32_t* __restrict__ first,
                                                         uint32_t* __restrict__ state, uint32_t cap, uint32_t* __restrict__ blk, uint32_t* __restrict__ bnd,
                                                         uint32_t* __restrict__ flags, uint32_t round, uint32_t nwg) {
    __shared__ JdTables t;
    __shared__ uint8_t s_raw[4][kDhtBytes];
    __shared__ uint32_t s_words[kWgLds];
    __shared__ uint32_t s_end[2][kSyncThreads];
    __shared__ uint32_t s_base;
    const uint32_t tid = threadIdx.x, g = blockIdx.x, i = g * kSyncThreads + tid;
    if (round == 0 && g == 0)
        for (uint32_t r = tid; r <= nwg; r += kSyncThreads) flags[r] = 0;
    if (round >= 2 && flags[round - 1] == 0) return;                        // uniform: the launch before this one changed nothing
    load_tables(t, s_raw, a);
    const WgStream w = make_scan(a, words, stream_words, s_words, s_base, start, first, i);
    const bool follows = w.live && w.sub.local > 0;                         // the start is the end of subsequence i - 1
    uint32_t* s_pos = state + i;
    uint32_t* s_sk = state + cap + i;
    uint32_t* e_pos = state + 2 * (size_t)cap + i;
    uint32_t* e_sk = state + 3 * (size_t)cap + i;
    JdState st, en;
    uint32_t done;
    bool changed, moved = false;
    if (round == 0) {
        st.pos = w.sub.lo, st.slot = 0, st.k = 0;
        en = st, done = 0;
        changed = w.live;
    } else {
        st.pos = *s_pos, st.slot = *s_sk >> 8, st.k = *s_sk & 255u;
        en.pos = *e_pos, en.slot = *e_sk >> 8, en.k = *e_sk & 255u;
        done = blk[i];
        changed = false;
        if (tid == 0 && g > 0 && follows) {
            const uint32_t* b = bnd + ((size_t)((round - 1) & 1u) * nwg + (g - 1)) * 2;
            const uint32_t p = b[0], sk = b[1];
            changed = p != st.pos || sk != ((st.slot << 8) | st.k);
            st.pos = p, st.slot = sk >> 8, st.k = sk & 255u;
        }
    }
    // thread t is final after t rounds of the loop: the bound is the number of subsequences of the workgroup
    for (uint32_t it = 0; it <= kSyncThreads; ++it) {
        if (changed) {
            en = st;
            done = jd_run(w.sc, t, en, w.sub.limit, 0u, JdNoSink());
        }
        s_end[0][tid] = en.pos, s_end[1][tid] = (en.slot << 8) | en.k;
        __syncthreads();
        changed = false;
        if (tid > 0 && follows) {
            const uint32_t p = s_end[0][tid - 1], sk = s_end[1][tid - 1];
            changed = p != st.pos || sk != ((st.slot << 8) | st.k);
            st.pos = p, st.slot = sk >> 8, st.k = sk & 255u;
        }
        if (!__syncthreads_or(changed)) break;
    }
    *s_pos = st.pos, *s_sk = (st.slot << 8) | st.k;
    *e_pos = en.pos, *e_sk = (en.slot << 8) | en.k;
    blk[i] = done;
    if (tid == kSyncThreads - 1) {
        uint32_t* b = bnd + ((size_t)(round & 1u) * nwg + g) * 2;
        const uint32_t sk = (en.slot << 8) | en.k;
        if (round > 0) {                                                    // the next launch reads nothing else that this one wrote
            const uint32_t* was = bnd + ((size_t)((round - 1) & 1u) * nwg + g) * 2;
            moved = was[0] != en.pos || was[1] != sk;
        }
        b[0] = en.pos, b[1] = sk;
    }
    if (round > 0 && __syncthreads_or(moved) && tid == 0) atomicOr(flags + round, 1u);
}

struct CoefSink {
    int16_t* coef;
    uint32_t blk_end;                                                    // of the interval; a subsequence's first block is never in front of it
    __device__ __forceinline__ void operator()(uint32_t block, uint32_t k, int v) const {
        if (block < blk_end) coef[(size_t)block * 64 + g_nat.v[k & 63u]] = (int16_t)v;
    }
};

// blk: the exclusive prefix sum of the blocks completed per subsequence, blk[cap] their sum
__global__ __launch_bounds__(256) void jpegr_write_kernel(const RScanArgs a, const uint32_t* __restrict__ words, uint32_t stream_words,
                                                          const uint32_t* __restrict__ start, const uint32_t* __restrict__ first,
                                                          const uint32_t* __restrict__ state, uint32_t cap, const uint32_t* __restrict__ blk,
                                                          int16_t* __restrict__ coef, int32_t* __restrict__ status) {
    __shared__ JdTables t;
    __shared__ uint8_t s_raw[4][kDhtBytes];
    __shared__ uint32_t s_words[kWgLds];
    __shared__ uint32_t s_base;
    load_tables(t, s_raw, a);
    const uint32_t i = blockIdx.x * kSyncThreads + threadIdx.x;
    const WgStream w = make_scan(a, words, stream_words, s_words, s_base, start, first, i);
    if (!w.live) return;
    const uint32_t before = blk[first[w.sub.ivl]];                       // blocks in front of the interval's first subsequence
    JdState st;
    st.pos = state[i], st.slot = state[cap + i] >> 8, st.k = state[cap + i] & 255u;
    jd_run(w.sc, t, st, w.sub.limit, w.sub.blk0 + (blk[i] - before), CoefSink{coef, w.sub.blk_end});
    if (w.sub.local == 0) {
        const uint32_t got = blk[first[w.sub.ivl + 1]] - before, want = w.sub.blk_end - w.sub.blk0;       // first[nint] <= cap
        if (got != want) atomicOr(status, got < want ? 1 : 2);
    }
}

// ---- DC prediction --------------------------------------------------------------------------------------------------------------
// the prefix sum of csrc/jpeg_dec.hip's jpegd_dc_kernel over (head, value) pairs: a head -- a component's first block of an interval --
// starts a new sum
__global__ __launch_bounds__(1024) void jpegr_dc_kernel(int16_t* __restrict__ coef, uint32_t nmcu, uint32_t nb, uint32_t ny, uint32_t ri) {
    __shared__ int s_val[16], s_head[16];
    __shared__ int s_carry;
    const uint32_t c = blockIdx.x;
    const uint32_t n = c == 0 ? nmcu * ny : nmcu;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < n; base += 1024) {
        const uint32_t j = base + threadIdx.x;
        const uint32_t mcu = c == 0 ? j / ny : j, sub = c == 0 ? j % ny : 0u;
        const size_t b = (size_t)mcu * nb + (c == 0 ? sub : ny + c - 1);
        int inc = j < n ? (int)coef[b * 64] : 0;
        int head = j < n && sub == 0 && mcu % ri == 0 ? 1 : 0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(inc, o, 64), uph = __shfl_up(head, o, 64);
            if (lane >= o) {
                if (!head) inc += up;
                head |= uph;
            }
        }
        if (lane == 63) s_val[wv] = inc, s_head[wv] = head;
        __syncthreads();
        int before = s_carry;
        for (int k = 0; k < wv; ++k) before = s_head[k] ? s_val[k] : before + s_val[k];
        const int v = head ? inc : before + inc;
        if (j < n) coef[b * 64] = (int16_t)v;
        __syncthreads();
        if (threadIdx.x == 1023) s_carry = v;
        __syncthreads();
    }
}

// ---- encoder ----------------------------------------------------------------------------------------------------------------------
// the DC value block b is predicted from: its scan-order predecessor in the component, 0 at the start of the scan and of an interval
__device__ __forceinline__ int rst_pred(const int16_t* __restrict__ coef, uint32_t b, uint32_t nb, uint32_t ny, uint32_t ri, int& table) {
    const int64_t pb = block_pred(b, nb, ny, table);
    if (pb < 0 || ((uint32_t)pb / nb) / ri != (b / nb) / ri) return 0;
    return (int)coef[pb * 64];
}

__global__ __launch_bounds__(256) void jpegr_enc_hist_kernel(const int16_t* __restrict__ coef, uint32_t* __restrict__ hist, uint32_t nblocks, uint32_t nb, uint32_t ny,
                                                             uint32_t ri) {
    __shared__ uint32_t s_hist[4 * kJhEntries];
    for (int i = threadIdx.x; i < 4 * kJhEntries; i += 256) s_hist[i] = 0u;
    __syncthreads();
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b < nblocks) {
        int t;
        const int pred = rst_pred(coef, b, nb, ny, ri, t);
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

__global__ __launch_bounds__(256) void jpegr_enc_bits_kernel(const int16_t* __restrict__ coef, uint32_t* __restrict__ len, const JDev* __restrict__ dev, uint32_t nblocks,
                                                             uint32_t nb, uint32_t ny, uint32_t ri) {
    __shared__ HuffLds h;
    load_huff(h, dev ? &dev->tabs : &g_std);
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nblocks) return;
    int t;
    const int pred = rst_pred(coef, b, nb, ny, ri, t);
    uint32_t bits = 0;
    walk_block(
        coef, b, pred, [&](int n, int) { bits += (h.dc[t][n & 15] >> 16) + n; }, [&](int k) { bits += (uint32_t)k * (h.ac[t][0xF0] >> 16); },
        [&](int sym, int, int n) { bits += (h.ac[t][sym & 255] >> 16) + n; });
    len[b] = bits;
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

__global__ __launch_bounds__(256) void jpegr_enc_pack_kernel(const int16_t* __restrict__ coef, const uint32_t* __restrict__ off, uint32_t* __restrict__ stream,
                                                             uint32_t cap_words, const JDev* __restrict__ dev, uint32_t nblocks, uint32_t nb, uint32_t ny, uint32_t ri) {
    __shared__ HuffLds h;
    load_huff(h, dev ? &dev->tabs : &g_std);
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nblocks) return;
    int t;
    const int pred = rst_pred(coef, b, nb, ny, ri, t);
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
    if (b + 1 == nblocks || (b + 1) % (ri * nb) == 0) {                 // the interval's final partial byte is padded with 1-bits (words are byte multiples)
        const int pad = (8 - (w.n & 7)) & 7;
        put_bits(w, (1u << pad) - 1u, pad);
    }
    if (w.n > 0 && w.word < w.end) atomicOr(w.word, __builtin_bswap32((uint32_t)(w.acc << (32 - w.n))));
}

// ibyte[1 .. nint - 1]: strictly increasing (an interval holds at least one block, a block at least two bits, and ends on a byte)
__global__ __launch_bounds__(256) void jpegr_enc_stuff_kernel(const uint32_t* __restrict__ stream, const uint32_t* __restrict__ totals, const uint32_t* __restrict__ cnt_off,
                                                              const uint32_t* __restrict__ ibyte, uint32_t nint, uint32_t ri, uint8_t* __restrict__ out,
                                                              int32_t* __restrict__ out_nbytes, const JHeader hp, const JDev* __restrict__ dev) {
    __shared__ uint32_t s_wave[4];
    const JTabs* tabs = dev ? &dev->tabs : &g_std;
    const uint32_t nbytes = (totals[0] + 7u) >> 3;
    const uint32_t hdr0 = dev ? header_bytes(hp.ncomp, dev->tabs) : hp.std_bytes, hdr = hdr0 + 6u;
    if (blockIdx.x == gridDim.x - 1) {
        write_header(out, hp, tabs);
        if (threadIdx.x == 0) {                                         // (this thread wrote SOS: it moves six bytes back, DRI takes its place)
            const uint32_t sos = 8u + 2u * (uint32_t)hp.ncomp;
            uint8_t* h = out + hdr0 - sos;
            for (int k = (int)sos - 1; k >= 0; --k) h[k + 6] = h[k];
            h[0] = 0xFF, h[1] = 0xDD, h[2] = 0, h[3] = 4, h[4] = (uint8_t)(ri >> 8), h[5] = (uint8_t)(ri & 255u);
            const uint32_t end = hdr + nbytes + totals[1] + 2u * (nint - 1u);
            out[end] = 0xFF, out[end + 1] = 0xD9;
            *out_nbytes = (int32_t)(end + 2);
        }
    }
    if (blockIdx.x * kChunk >= nbytes) return;
    const uint32_t i0 = blockIdx.x * kChunk + threadIdx.x * 8;
    const uint2 d = i0 < nbytes ? *(const uint2*)(stream + (i0 >> 2)) : make_uint2(0u, 0u);
    uint32_t ex;
    block_sum_256(ff_bytes(d, i0, nbytes), ex, s_wave);
    uint32_t lo = 0, hi = nint;                                         // m: the intervals 1 .. nint - 1 that start in front of byte i0
    while (hi - lo > 1u) {                                              // ibyte[lo] < i0 or lo == 0; ibyte[hi] >= i0 or hi == nint
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (ibyte[mid] < i0) lo = mid;
        else hi = mid;
    }
    uint32_t m = lo;
    uint8_t* o = out + hdr + i0 + cnt_off[blockIdx.x] + ex + 2u * m;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t byte = ((k < 4 ? d.x : d.y) >> ((k & 3) * 8)) & 255u;
        if (i0 + k < nbytes) {
            if (m + 1u < nint && ibyte[m + 1u] == i0 + k) {
                *o++ = 0xFF, *o++ = (uint8_t)(0xD0u + (m & 7u));
                ++m;
            }
            *o++ = (uint8_t)byte;
            if (byte == 255u) *o++ = 0;
        }
    }
}

}  // namespace

size_t st_jpeg_rst_workspace_bytes(uint32_t scan_len, uint32_t nmcu, uint32_t ri) { return make_geom(scan_len, nmcu, ri).bytes; }

int st_jpeg_rst_entropy(const JpegRstDecode& d) {
    const RGeom g = make_geom(d.scan_len, d.nmcu, d.ri);
    hipStream_t st = d.st;
    char* ws = (char*)d.ws;
    uint32_t* tot = (uint32_t*)ws;
    uint32_t* ndrop = (uint32_t*)(ws + g.off_drop);
    uint32_t* nmark = (uint32_t*)(ws + g.off_nmark);
    uint32_t* mark_pos = (uint32_t*)(ws + g.off_mark);
    uint32_t* start = (uint32_t*)(ws + g.off_start);
    uint32_t* first = (uint32_t*)(ws + g.off_first);
    uint32_t* state = (uint32_t*)(ws + g.off_state);
    uint32_t* blk = (uint32_t*)(ws + g.off_blk);
    uint32_t* bnd = (uint32_t*)(ws + g.off_bnd);
    uint32_t* flags = (uint32_t*)(ws + g.off_flags);
    RScanArgs a;
    a.file = d.file, a.nbytes = d.nbytes;
    for (int i = 0; i < 2; ++i) a.dc_off[i] = d.dc_off[i], a.ac_off[i] = d.ac_off[i];
    a.nb = d.nb, a.ny = d.ny, a.td_bits = d.td_bits, a.ta_bits = d.ta_bits;
    a.nmcu = d.nmcu, a.ri = d.ri, a.nint = g.nint;
    const uint8_t* scan = d.file + d.scan_off;
    const uint32_t* words = (const uint32_t*)d.stream;

    hipLaunchKernelGGL(jpegr_count_kernel, dim3(g.nchunks), dim3(256), 0, st, scan, d.scan_len, ndrop, nmark);
    ST_CHECK_LAUNCH();
    hipError_t e = st_jpeg_scan_u32(ndrop, g.nchunks, tot, st);
    if (e != hipSuccess) return (int)e;
    e = st_jpeg_scan_u32(nmark, g.nchunks, tot + 1, st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(jpegr_unstuff_kernel, dim3(g.nchunks), dim3(256), 0, st, scan, d.scan_len, (const uint32_t*)ndrop, (const uint32_t*)nmark, (const uint32_t*)tot, d.stream,
                       mark_pos, g.nint);
    ST_CHECK_LAUNCH();
    hipLaunchKernelGGL(jpegr_cut_kernel, dim3((g.nint + 255) / 256), dim3(256), 0, st, (const uint32_t*)mark_pos, (const uint32_t*)tot, d.scan_len, g.nint, start, first, d.status);
    ST_CHECK_LAUNCH();
    e = st_jpeg_scan_u32(first, g.nint, first + g.nint, st);
    if (e != hipSuccess) return (int)e;
    for (uint32_t r = 0; r < g.nwg; ++r) {
        hipLaunchKernelGGL(jpegr_sync_kernel, dim3(g.nwg), dim3(kSyncThreads), 0, st, a, words, d.stream_words, (const uint32_t*)start, (const uint32_t*)first, state, g.cap, blk,
                           bnd, flags, r, g.nwg);
        ST_CHECK_LAUNCH();
    }
    e = st_jpeg_scan_u32(blk, g.cap, blk + g.cap, st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(jpegr_write_kernel, dim3(g.nwg), dim3(kSyncThreads), 0, st, a, words, d.stream_words, (const uint32_t*)start, (const uint32_t*)first, (const uint32_t*)state,
                       g.cap, (const uint32_t*)blk, d.coef, d.status);
    ST_CHECK_LAUNCH();
    hipLaunchKernelGGL(jpegr_dc_kernel, dim3(d.nb > 1 ? 3 : 1), dim3(1024), 0, st, d.coef, d.nmcu, d.nb, d.ny, d.ri);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

int st_jpeg_rst_hist(const JpegRstEncode& e) {
    hipLaunchKernelGGL(jpegr_enc_hist_kernel, dim3((e.nblocks + 255) / 256), dim3(256), 0, e.st, e.coef, &((JDev*)e.dev)->hist[0][0], e.nblocks, e.nb, e.ny, e.ri);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

int st_jpeg_rst_offsets(const JpegRstEncode& e) {
    const uint32_t per = e.ri * e.nb;
    hipLaunchKernelGGL(jpegr_enc_bits_kernel, dim3((e.nblocks + 255) / 256), dim3(256), 0, e.st, e.coef, e.len, (const JDev*)e.dev, e.nblocks, e.nb, e.ny, e.ri);
    ST_CHECK_LAUNCH();
    hipError_t err = st_jpeg_scan_u32(e.len, e.nblocks, e.tot, e.st);
    if (err != hipSuccess) return (int)err;
    hipLaunchKernelGGL(jpegr_enc_pad_kernel, dim3((e.nint + 255) / 256), dim3(256), 0, e.st, (const uint32_t*)e.len, (const uint32_t*)e.tot, e.pad, e.nblocks, per, e.nint);
    ST_CHECK_LAUNCH();
    err = st_jpeg_scan_u32(e.pad, e.nint, e.tot + 2, e.st);
    if (err != hipSuccess) return (int)err;
    hipLaunchKernelGGL(jpegr_enc_offsets_kernel, dim3((e.nblocks + 255) / 256), dim3(256), 0, e.st, e.len, e.tot, (const uint32_t*)e.pad, e.ibyte, e.nblocks, per);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

int st_jpeg_rst_pack(const JpegRstEncode& e) {
    hipLaunchKernelGGL(jpegr_enc_pack_kernel, dim3((e.nblocks + 255) / 256), dim3(256), 0, e.st, e.coef, (const uint32_t*)e.len, e.stream, e.stream_words, (const JDev*)e.dev,
                       e.nblocks, e.nb, e.ny, e.ri);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

int st_jpeg_rst_stuff(const JpegRstEncode& e) {
    hipLaunchKernelGGL(jpegr_enc_stuff_kernel, dim3(e.nchunks), dim3(256), 0, e.st, (const uint32_t*)e.stream, (const uint32_t*)e.tot, e.cnt, (const uint32_t*)e.ibyte, e.nint, e.ri,
                       e.out, e.out_nbytes, *(const JHeader*)e.header, (const JDev*)e.dev);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

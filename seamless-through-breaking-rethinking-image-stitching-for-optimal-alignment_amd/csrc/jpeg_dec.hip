// Baseline JPEG decoder for the input files of evaluate.py and out.py (`PIL.Image.open(path)` on the reference's worker threads): the
// uint8 [H, W, C] array Pillow returns on libjpeg-turbo at its defaults -- Huffman baseline, integer "islow" IDCT, fancy upsampling, the
// fixed-point YCbCr -> RGB of jdcolor.c -- bit for bit (contract: README.md; CPU restatement: tests/_jpeg_dec_ref.py).  Integer arithmetic
// only.  The host parses the markers (ops.jpeg_probe) and passes offsets; the tables are read on the device from the file's bytes.
//
//   jpegd_count_kernel    stuffed 0x00 bytes (a 0x00 behind a 0xFF) per 2048-byte chunk of the scan; jpeg_scan_kernel (csrc/jpeg.hip) scans them
//   jpegd_unstuff_kernel  compacts the scan to the unstuffed stream, 16 zero bytes behind it
//   jpegd_sync_kernel     one thread per subsequence of 1024 bits: decodes from a guessed state (bit i * 1024, slot 0, DC next), then the
//                         workgroup repeats `start[i] <- end[i - 1]` to its fixpoint; launched once per workgroup of subsequences, each later
//                         launch carries one more workgroup boundary and returns at once when the launch before it changed nothing
//   jpeg_scan_kernel      blocks completed per subsequence -> first block of every subsequence, total
//   jpegd_zero_kernel     clears the int16 [nblocks, 64] coefficients (part of the call: a reused workspace is fine)
//   jpegd_write_kernel    decodes every subsequence again from its final state and writes the coefficients it meets (natural order, DC
//                         differences) into the zeroed int16 [nblocks, 64]; sets the status word
//   jpegd_dc_kernel       one workgroup per component: prefix sum of the DC differences
//   jpegd_idct_kernel     one wave per 8 blocks: dequantisation, column and row pass of jidctint.c through LDS, range limit -> sample planes
//   jpegd_pixels_kernel   one thread per pixel: fancy h2v1 / h2v2 upsampling (replication at chroma width <= 2), colour conversion, HWC store
//
// A file with restart intervals (st_jpeg_dec_params.restart_interval > 0; contract: README.md "Restart intervals"; CPU restatement:
// tests/_jpeg_rst_ref.py; the cutting rules in plain C++: csrc/jpeg_rst_core.h) shares the zero, IDCT and pixel kernels.  An interval starts
// byte-aligned behind a marker that cannot occur in the data, with DC predictions 0 and at a known MCU: no decoder state is guessed at its
// start and nothing crosses from one interval to the next.  The count, unstuff and DC steps are each written once, as a body on `bool RST`,
// and the kernels of both paths are its two instantiations; the sync and write kernels stand beside their plain twins (see there):
//
//   jpegr_count_kernel    per chunk also the bytes of the restart markers, which are not part of the stream either, and the markers themselves;
//                         jpeg_scan_kernel scans both
//   jpegr_unstuff_kernel  the unstuffed stream without its markers; writes the stream offset behind every marker
//   jpegr_cut_kernel      one thread per interval: its start in the stream and its number of 1024-bit subsequences; jpeg_scan_kernel makes
//                         the first subsequence of every interval from them.  Clears the status word
//   jpegr_sync_kernel     an interval's first subsequence decodes from its known state, the others from a guess (their first bit, slot 0, DC
//                         next); `start[j] <- end[j - 1]` runs inside every interval.  A later launch returns at once when the launch before it
//                         moved no workgroup's end state
//   jpegr_write_kernel    writes the coefficients into its interval's blocks only; an interval whose bytes held another number of blocks than it
//                         has sets bit 0 (fewer) or bit 1 (more) of the status
//   jpegr_dc_kernel       the prefix sum of the DC differences restarts at every interval
#include "common.h"
#include "jpeg_dec_core.h"
#include "jpeg_rst_core.h"
#include "jpeg_scan.h"
#include "jpeg_tables.h"
#include "../../include/stitch_gfx950.h"

namespace {

struct NatTable {
    uint8_t v[64];                                       // zigzag position -> natural index
};
constexpr NatTable make_nat() {
    NatTable t{};
    for (int i = 0; i < 64; ++i) t.v[i] = (uint8_t)kZigzag[i];
    return t;
}
__device__ const NatTable g_nat = make_nat();

constexpr int64_t kMaxPixels = (int64_t)1 << 24;
constexpr int64_t kMaxFileBytes = (int64_t)1 << 28;      // bit positions stay below 2^31
constexpr uint32_t kChunk = 2048;                        // scan bytes per workgroup of the unstuffing passes (256 threads x 8 bytes)
constexpr uint32_t kSubBits = kJrSubBits;                // bits per subsequence (one thread)
constexpr uint32_t kSyncThreads = 256;                   // subsequences per workgroup
constexpr uint32_t kPad = 16;                            // zero bytes behind the unstuffed stream
constexpr int kWorkLd = 72;                              // dwords per block between the IDCT passes (csrc/jpeg.hip: 64 + 8)

struct DGeom {
    int32_t H, W, ncomp, hs, vs, stride;
    int32_t mcu_rows, mcu_cols;
    uint32_t nb, ny, nblocks;
    uint32_t scan_len, nchunks, nsub, nwg;
    int32_t yw, yh, cw, ch;          // padded plane sizes (luma, chroma)
    int32_t ccw, cch;                // cropped chroma size: ceil(W / hs) x ceil(H / vs)
    size_t off_cnt, off_stream, off_state, off_bnd, off_flags, off_coef, off_planes, ws_bytes;
};

inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

bool make_geom(int32_t H, int32_t W, int32_t ncomp, int32_t hs, int32_t vs, int64_t scan_len, DGeom& g) {
    if ((ncomp != 1 && ncomp != 3) || H < 1 || H > 65535 || W < 1 || W > 65535 || (int64_t)H * W > kMaxPixels) return false;
    if (!((hs == 1 && vs == 1) || (ncomp == 3 && hs == 2 && (vs == 1 || vs == 2)))) return false;
    if (scan_len < 1 || scan_len > kMaxFileBytes) return false;
    g.H = H, g.W = W, g.ncomp = ncomp, g.hs = hs, g.vs = vs, g.stride = 0;
    g.mcu_rows = (H + 8 * vs - 1) / (8 * vs), g.mcu_cols = (W + 8 * hs - 1) / (8 * hs);
    g.ny = ncomp == 3 ? (uint32_t)(hs * vs) : 1u;
    g.nb = ncomp == 3 ? g.ny + 2u : 1u;
    g.nblocks = (uint32_t)g.mcu_rows * (uint32_t)g.mcu_cols * g.nb;
    g.scan_len = (uint32_t)scan_len;
    g.nchunks = (g.scan_len + kChunk - 1) / kChunk;
    g.nsub = (uint32_t)(((uint64_t)g.scan_len * 8 + kSubBits - 1) / kSubBits);
    g.nwg = (g.nsub + kSyncThreads - 1) / kSyncThreads;
    g.yw = g.mcu_cols * hs * 8, g.yh = g.mcu_rows * vs * 8;
    g.cw = g.mcu_cols * 8, g.ch = g.mcu_rows * 8;
    g.ccw = (W + hs - 1) / hs, g.cch = (H + vs - 1) / vs;
    size_t o = 16;                                                         // totals: [0] stuffed bytes, [1] blocks in the stream
    g.off_cnt = o, o += align16((size_t)g.nchunks * 4);
    g.off_stream = o, o += align16((size_t)g.scan_len + kPad);
    g.off_state = o, o += 5 * align16((size_t)g.nwg * kSyncThreads * 4);   // start pos, start slot | k, end pos, end slot | k, blocks
    g.off_bnd = o, o += align16((size_t)g.nwg * 2 * 2 * 4);
    g.off_flags = o, o += align16((size_t)(g.nwg + 1) * 4);
    g.off_coef = o, o += align16((size_t)g.nblocks * 128);
    g.off_planes = o, o += align16((size_t)g.yw * g.yh + (ncomp == 3 ? 2 * (size_t)g.cw * g.ch : 0));
    g.ws_bytes = o;
    return true;
}

// what a file with restart intervals needs behind the plain layout: nint = ceil(nmcu / ri) intervals
struct RGeom {
    uint32_t nint, nchunks, cap, nwg;
    size_t off_drop, off_nmark, off_mark, off_start, off_first, off_state, off_blk, off_bnd, off_flags, bytes;
};

RGeom make_rst_geom(uint32_t scan_len, uint32_t nmcu, uint32_t ri) {
    RGeom g;
    g.nint = (nmcu + ri - 1) / ri;
    g.nchunks = (scan_len + kChunk - 1) / kChunk;
    // an interval of b bytes has max(1, ceil(8 b / 1024)) <= 8 b / 1024 + 1 subsequences
    const uint32_t nsub = (uint32_t)(((uint64_t)scan_len * 8 + kSubBits - 1) / kSubBits) + g.nint;
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
// The count and unstuff steps (and the DC step below) follow, each as one body for a plain file (RST false) and a file with restart intervals
// (RST true); what the other path's kernel has no argument for is passed as 0 / nullptr and never read.
//
// the 8 scan bytes from i0 and the byte before them; bit k of `drop`: byte i0 + k is not part of the stream -- a stuffed 0x00 (a 0x00 behind
// a 0xFF) and, RST only, the 0xFF or the 0xD0..0xD7 of a restart marker (then the byte behind the 8 is read too); bit k of `mark`, RST
// only: it is the second byte of a restart marker.  A plain scan has no markers and takes FF D0..D7 as data.
template <bool RST>
__device__ __forceinline__ void scan_masks(const uint8_t* __restrict__ scan, uint32_t i0, uint32_t n, uint8_t (&b)[8], uint32_t& drop, uint32_t& mark) {
    uint32_t prev = (i0 > 0 && i0 <= n) ? scan[i0 - 1] : 0u;
    uint32_t d = 0, m = 0;
    if constexpr (RST) {
        const uint32_t behind = (i0 + 8 < n) ? scan[i0 + 8] : 0u;
#pragma unroll
        for (int k = 0; k < 8; ++k) b[k] = i0 + k < n ? scan[i0 + k] : (uint8_t)1;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t next = k < 7 ? (uint32_t)b[(k + 1) & 7] : behind;
            if (i0 + k < n) {
                const uint32_t c = jr_byte_class(prev, b[k], next);
                d |= (c & 1u) << k, m |= (c >> 1) << k;
            }
            prev = b[k];
        }
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            b[k] = i0 + k < n ? scan[i0 + k] : (uint8_t)1;
            if (i0 + k < n && b[k] == 0 && prev == 255u) d |= 1u << k;
            prev = b[k];
        }
    }
    drop = d, mark = m;
}

// per chunk: the bytes that are not part of the stream and, RST only, the restart markers
template <bool RST>
__device__ __forceinline__ void count_body(const uint8_t* __restrict__ scan, uint32_t n, uint32_t* __restrict__ ndrop, uint32_t* __restrict__ nmark) {
    __shared__ uint32_t s_a[4], s_b[4];
    uint8_t b[8];
    uint32_t drop, mark, ex;
    scan_masks<RST>(scan, blockIdx.x * kChunk + threadIdx.x * 8, n, b, drop, mark);
    const uint32_t d = block_sum_256(__popc(drop), ex, s_a);
    if constexpr (RST) {
        const uint32_t m = block_sum_256(__popc(mark), ex, s_b);
        if (threadIdx.x == 0) ndrop[blockIdx.x] = d, nmark[blockIdx.x] = m;
    } else {
        if (threadIdx.x == 0) ndrop[blockIdx.x] = d;
    }
}

__global__ __launch_bounds__(256) void jpegd_count_kernel(const uint8_t* __restrict__ scan, uint32_t n, uint32_t* __restrict__ cnt) {
    count_body<false>(scan, n, cnt, nullptr);
}

__global__ __launch_bounds__(256) void jpegr_count_kernel(const uint8_t* __restrict__ scan, uint32_t n, uint32_t* __restrict__ ndrop, uint32_t* __restrict__ nmark) {
    count_body<true>(scan, n, ndrop, nmark);
}

// RST: mark_pos[i], i = 1 .. nint - 1: the stream offset behind the i-th marker (a marker past the last interval's is dropped and forgotten)
template <bool RST>
__device__ __forceinline__ void unstuff_body(const uint8_t* __restrict__ scan, uint32_t n, const uint32_t* __restrict__ drop_off, const uint32_t* __restrict__ mark_off,
                                             const uint32_t* __restrict__ tot, uint8_t* __restrict__ dst, uint32_t* __restrict__ mark_pos, uint32_t nint) {
    __shared__ uint32_t s_a[4], s_b[4];
    uint8_t b[8];
    const uint32_t i0 = blockIdx.x * kChunk + threadIdx.x * 8;
    uint32_t drop, mark, ex_d, ex_m;
    scan_masks<RST>(scan, i0, n, b, drop, mark);
    block_sum_256(__popc(drop), ex_d, s_a);
    if constexpr (RST) block_sum_256(__popc(mark), ex_m, s_b);
    if (i0 < n) {
        uint32_t o = i0 - drop_off[blockIdx.x] - ex_d;                  // kept bytes in front of byte i0: never more than i0
        uint32_t m = RST ? mark_off[blockIdx.x] + ex_m + 1 : 0u;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (i0 + k < n && !((drop >> k) & 1u)) dst[o++] = b[k];
            if constexpr (RST) {
                if ((mark >> k) & 1u) {
                    if (m < nint) mark_pos[m] = o;
                    ++m;
                }
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < kPad) dst[n - tot[0] + threadIdx.x] = 0;
}

__global__ __launch_bounds__(256) void jpegd_unstuff_kernel(const uint8_t* __restrict__ scan, uint32_t n, const uint32_t* __restrict__ cnt_off,
                                                            const uint32_t* __restrict__ tot, uint8_t* __restrict__ dst) {
    unstuff_body<false>(scan, n, cnt_off, nullptr, tot, dst, nullptr, 0u);
}

__global__ __launch_bounds__(256) void jpegr_unstuff_kernel(const uint8_t* __restrict__ scan, uint32_t n, const uint32_t* __restrict__ drop_off,
                                                            const uint32_t* __restrict__ mark_off, const uint32_t* __restrict__ tot, uint8_t* __restrict__ dst,
                                                            uint32_t* __restrict__ mark_pos, uint32_t nint) {
    unstuff_body<true>(scan, n, drop_off, mark_off, tot, dst, mark_pos, nint);
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
// What the sync and write kernels get by value: the tables' places in the file and the MCU's shape, then the plain path's two words or the
// restart path's three.  (Two types, not one with all five words: a kernel's symbol spells the types of its arguments, and the symbols are
// what tools/kernel_diff.py and the recorded profiles know the kernels by.)
struct DScanArgs {
    const uint8_t* file;
    uint32_t nbytes;
    uint32_t dc_off[2], ac_off[2];
    uint32_t nb, ny, td_bits, ta_bits;
    uint32_t scan_len, nblocks;
};
struct RScanArgs {
    const uint8_t* file;
    uint32_t nbytes;
    uint32_t dc_off[2], ac_off[2];
    uint32_t nb, ny, td_bits, ta_bits;
    uint32_t nmcu, ri, nint;
};

constexpr uint32_t kDhtBytes = 16 + 256;       // a DHT payload: the code counts, then at most 256 values

// the four DHT payloads come into LDS with one coalesced pass (bytes past the end of the file read as 0), then four threads build the
// decode tables from there: built straight from global memory, the ~300 dependent byte loads per table cost 0.2 ms per launch
template <class Args>
__device__ __forceinline__ void load_tables(JdTables& t, uint8_t (&raw)[4][kDhtBytes], const Args& a) {
    for (uint32_t i = threadIdx.x; i < 4 * kDhtBytes; i += blockDim.x) {
        const uint32_t tab = i / kDhtBytes, j = i - tab * kDhtBytes;
        const uint32_t off = tab == 0 ? a.dc_off[0] : tab == 1 ? a.dc_off[1] : tab == 2 ? a.ac_off[0] : a.ac_off[1];     // constant indices
        raw[tab][j] = (off < a.nbytes && j < a.nbytes - off) ? a.file[off + j] : (uint8_t)0;
    }
    __syncthreads();
    if (threadIdx.x < 4) jd_build_huff(threadIdx.x < 2 ? t.dc[threadIdx.x] : t.ac[threadIdx.x - 2], raw[threadIdx.x], kDhtBytes, 0u);
    __syncthreads();
}

constexpr uint32_t kWgWords = kSyncThreads * kSubBits / 32;      // stream words a workgroup's subsequences cover
constexpr uint32_t kWgLds = kWgWords + 4;                        // + the word its first bit starts in + the two words a symbol that starts in the last bit reaches into

// The sync and write kernels stand twice, for a plain file (jpegd_*) and for restart intervals (jpegr_*): written once as a function
// template they compile to other code, and the plain decode of a 512x512 file measured 5 % slower (profiles/jpeg_rst_unify_bench.json).
// They share the state load and store, the fixpoint loop, the boundary hand-over and the flag protocol; they differ in where a
// subsequence starts, whether it follows its neighbour, its limits, and in what raises flags[round].
//
// The workgroup's part of the stream comes into LDS with one coalesced pass: a thread reads bits from (i * 1024 or later) up to 64
// bits past ((i + 1) * 1024 - 1), all inside [g * 256 * 1024, (g + 1) * 256 * 1024 + 64).  Decoding from global memory made every
// symbol wait for two dependent loads.  Words past the stream's buffer (stream_words) read as 0.
__device__ __forceinline__ JdScan make_scan(const DScanArgs& a, const uint32_t* __restrict__ words, uint32_t stream_words, uint32_t (&lds)[kWgLds],
                                            const uint32_t* tot) {
    const uint32_t base = blockIdx.x * kWgWords;
    for (uint32_t j = threadIdx.x; j < kWgLds; j += blockDim.x) lds[j] = base + j < stream_words ? words[base + j] : 0u;
    __syncthreads();
    JdScan sc;
    sc.words = lds, sc.base_word = base;
    sc.nbits = 8u * (a.scan_len - tot[0]);
    sc.nb = a.nb, sc.ny = a.ny;
    sc.td_bits = a.td_bits, sc.ta_bits = a.ta_bits;
    return sc;
}

// state arrays: [5][cap] -- start pos, start (slot << 8 | k), end pos, end (slot << 8 | k), blocks completed
// bnd: [2][nwg][2] the end state of every workgroup's last subsequence, written by launch r into half r & 1
// flags: [nwg + 1], flags[r] != 0: launch r changed a start
__global__ __launch_bounds__(256) void jpegd_sync_kernel(const DScanArgs a, const uint32_t* __restrict__ words, uint32_t stream_words,
                                                         const uint32_t* __restrict__ tot,
                                                         uint32_t* __restrict__ state, uint32_t cap, uint32_t* __restrict__ bnd, uint32_t* __restrict__ flags,
                                                         uint32_t round, uint32_t nwg) {
    __shared__ JdTables t;
    __shared__ uint8_t s_raw[4][kDhtBytes];
    __shared__ uint32_t s_words[kWgLds];
    __shared__ uint32_t s_end[2][kSyncThreads];
    const uint32_t tid = threadIdx.x, g = blockIdx.x, i = g * kSyncThreads + tid;
    if (round == 0 && g == 0)
        for (uint32_t r = tid; r <= nwg; r += kSyncThreads) flags[r] = 0;
    if (round >= 2 && flags[round - 1] == 0) return;                        // uniform: the launch before this one changed nothing
    load_tables(t, s_raw, a);
    const JdScan sc = make_scan(a, words, stream_words, s_words, tot);
    uint32_t* s_pos = state + i;
    uint32_t* s_sk = state + cap + i;
    uint32_t* e_pos = state + 2 * (size_t)cap + i;
    uint32_t* e_sk = state + 3 * (size_t)cap + i;
    uint32_t* n_blk = state + 4 * (size_t)cap + i;
    JdState st, en;
    uint32_t done;
    bool changed, any = false;
    if (round == 0) {
        st.pos = i * kSubBits, st.slot = 0, st.k = 0;
        en = st, done = 0;
        changed = true;
    } else {
        st.pos = *s_pos, st.slot = *s_sk >> 8, st.k = *s_sk & 255u;
        en.pos = *e_pos, en.slot = *e_sk >> 8, en.k = *e_sk & 255u;
        done = *n_blk;
        changed = false;
        if (tid == 0 && g > 0) {
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
            done = jd_run(sc, t, en, (i + 1) * kSubBits, 0u, JdNoSink());
            any = any || it > 0 || round > 0;
        }
        s_end[0][tid] = en.pos, s_end[1][tid] = (en.slot << 8) | en.k;
        __syncthreads();
        changed = false;
        if (tid > 0) {
            const uint32_t p = s_end[0][tid - 1], sk = s_end[1][tid - 1];
            changed = p != st.pos || sk != ((st.slot << 8) | st.k);
            st.pos = p, st.slot = sk >> 8, st.k = sk & 255u;
        }
        if (!__syncthreads_or(changed)) break;
    }
    *s_pos = st.pos, *s_sk = (st.slot << 8) | st.k;
    *e_pos = en.pos, *e_sk = (en.slot << 8) | en.k;
    *n_blk = done;
    if (tid == kSyncThreads - 1) {
        uint32_t* b = bnd + ((size_t)(round & 1u) * nwg + g) * 2;
        b[0] = en.pos, b[1] = (en.slot << 8) | en.k;
    }
    if (round > 0 && __syncthreads_or(any) && tid == 0) atomicOr(flags + round, 1u);
}

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

// (a kernel, not a memset: every entry point of the library may be captured into a graph)
__global__ __launch_bounds__(256) void jpegd_zero_kernel(uint4* __restrict__ dst, uint32_t n) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) dst[i] = make_uint4(0u, 0u, 0u, 0u);
}

struct CoefSink {
    int16_t* coef;
    uint32_t blk_end;                                                    // of the scan, with restart intervals: of the interval; a subsequence's first block is never in front of it
    __device__ __forceinline__ void operator()(uint32_t block, uint32_t k, int v) const {
        if (block < blk_end) coef[(size_t)block * 64 + g_nat.v[k & 63u]] = (int16_t)v;
    }
};

__global__ __launch_bounds__(256) void jpegd_write_kernel(const DScanArgs a, const uint32_t* __restrict__ words, uint32_t stream_words,
                                                          const uint32_t* __restrict__ tot,
                                                          const uint32_t* __restrict__ state, uint32_t cap, int16_t* __restrict__ coef,
                                                          int32_t* __restrict__ status) {
    __shared__ JdTables t;
    __shared__ uint8_t s_raw[4][kDhtBytes];
    __shared__ uint32_t s_words[kWgLds];
    load_tables(t, s_raw, a);
    const JdScan sc = make_scan(a, words, stream_words, s_words, tot);
    const uint32_t i = blockIdx.x * kSyncThreads + threadIdx.x;
    JdState st;
    st.pos = state[i], st.slot = state[cap + i] >> 8, st.k = state[cap + i] & 255u;
    jd_run(sc, t, st, (i + 1) * kSubBits, state[4 * (size_t)cap + i], CoefSink{coef, a.nblocks});
    if (i == 0) *status = tot[1] == a.nblocks ? 0 : (tot[1] < a.nblocks ? 1 : 2);
}

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
// one workgroup per component: the prefix sum of its DC differences in scan order.  RST: over (head, value) pairs -- a head, a
// component's first block of an interval, starts a new sum
template <bool RST>
__device__ __forceinline__ void dc_body(int16_t* __restrict__ coef, uint32_t nmcu, uint32_t nb, uint32_t ny, uint32_t ri) {
    __shared__ int s_val[16], s_head[RST ? 16 : 1];
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
        int head = RST && j < n && sub == 0 && mcu % ri == 0 ? 1 : 0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(inc, o, 64);
            int uph = 0;
            if constexpr (RST) uph = __shfl_up(head, o, 64);
            if (lane >= o) {
                if (!head) inc += up;
                head |= uph;
            }
        }
        if (lane == 63) {
            s_val[wv] = inc;
            if constexpr (RST) s_head[wv] = head;
        }
        __syncthreads();
        int before = s_carry;
        for (int k = 0; k < wv; ++k) before = RST && s_head[k] ? s_val[k] : before + s_val[k];
        const int v = head ? inc : before + inc;
        if (j < n) coef[b * 64] = (int16_t)v;
        __syncthreads();
        if (threadIdx.x == 1023) s_carry = v;
        __syncthreads();
    }
}

__global__ __launch_bounds__(1024) void jpegd_dc_kernel(int16_t* __restrict__ coef, uint32_t nmcu, uint32_t nb, uint32_t ny) { dc_body<false>(coef, nmcu, nb, ny, 0u); }

__global__ __launch_bounds__(1024) void jpegr_dc_kernel(int16_t* __restrict__ coef, uint32_t nmcu, uint32_t nb, uint32_t ny, uint32_t ri) {
    dc_body<true>(coef, nmcu, nb, ny, ri);
}

// ---- inverse DCT (jidctint.c "islow": CONST_BITS 13, PASS1_BITS 2) --------------------------------------------------------------
template <int SHIFT>
__device__ __forceinline__ void idct8(int (&d)[8]) {
    constexpr int RND = 1 << (SHIFT - 1);
    int z1 = (d[2] + d[6]) * 4433;
    const int e2 = z1 - d[6] * 15137, e3 = z1 + d[2] * 6270;
    const int e0 = (d[0] + d[4]) * 8192, e1 = (d[0] - d[4]) * 8192;
    const int t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
    int t0 = d[7], t1 = d[5], t2 = d[3], t3 = d[1];
    z1 = t0 + t3;
    int z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const int z5 = (z3 + z4) * 9633;
    t0 *= 2446, t1 *= 16819, t2 *= 25172, t3 *= 12299;
    z1 *= -7373, z2 *= -20995;
    z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
    t0 += z1 + z3, t1 += z2 + z4, t2 += z2 + z3, t3 += z1 + z4;
    d[0] = (t10 + t3 + RND) >> SHIFT, d[7] = (t10 - t3 + RND) >> SHIFT;
    d[1] = (t11 + t2 + RND) >> SHIFT, d[6] = (t11 - t2 + RND) >> SHIFT;
    d[2] = (t12 + t1 + RND) >> SHIFT, d[5] = (t12 - t1 + RND) >> SHIFT;
    d[3] = (t13 + t0 + RND) >> SHIFT, d[4] = (t13 - t0 + RND) >> SHIFT;
}

// libjpeg's masked range-limit table, centred on 128
__device__ __forceinline__ uint32_t range_limit(int v) {
    const int x = v & 1023;
    return (uint32_t)(x < 128 ? x + 128 : x < 512 ? 255 : x < 896 ? 0 : x - 896);
}

__global__ __launch_bounds__(256) void jpegd_idct_kernel(const int16_t* __restrict__ coef, const uint8_t* __restrict__ file, uint32_t q_off0, uint32_t q_off1,
                                                         uint32_t q_off2, uint8_t* __restrict__ planes, const DGeom g) {
    __shared__ int s_q[3][64];               // natural order
    __shared__ int s_work[4][8 * kWorkLd];
    if (threadIdx.x < 192) {
        const int c = threadIdx.x >> 6, z = threadIdx.x & 63;
        s_q[c][g_nat.v[z]] = file[(c == 0 ? q_off0 : c == 1 ? q_off1 : q_off2) + z];
    }
    __syncthreads();
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int blk = lane >> 3, rc = lane & 7;
    const uint32_t b = (blockIdx.x * 4 + wv) * 8 + blk;
    const bool live = b < g.nblocks;
    const uint32_t mcu = live ? b / g.nb : 0u, slot = live ? b - mcu * g.nb : 0u;
    const uint32_t comp = slot < g.ny ? 0u : slot - g.ny + 1u;
    int* work = s_work[wv] + blk * kWorkLd;
    if (live) {                                                      // columns
        int d[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = (int)coef[(size_t)b * 64 + k * 8 + rc] * s_q[comp][k * 8 + rc];
        idct8<11>(d);
#pragma unroll
        for (int k = 0; k < 8; ++k) work[k * 8 + rc] = d[k];
    }
    __syncthreads();
    if (!live) return;
    int d[8];                                                        // rows
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = work[rc * 8 + k];
    idct8<18>(d);
    const uint32_t my = mcu / (uint32_t)g.mcu_cols, mx = mcu - my * (uint32_t)g.mcu_cols;
    uint8_t* plane = planes;
    int pw = g.yw;
    uint32_t by = my, bx = mx;
    if (g.ncomp == 3) {
        if (comp == 0) {
            by = my * g.vs + slot / g.hs, bx = mx * g.hs + slot % g.hs;
        } else {
            plane += (size_t)g.yw * g.yh + (size_t)(comp - 1) * g.cw * g.ch;
            pw = g.cw;
        }
    }
    uint2 o;
    o.x = range_limit(d[0]) | (range_limit(d[1]) << 8) | (range_limit(d[2]) << 16) | (range_limit(d[3]) << 24);
    o.y = range_limit(d[4]) | (range_limit(d[5]) << 8) | (range_limit(d[6]) << 16) | (range_limit(d[7]) << 24);
    *(uint2*)(plane + ((size_t)by * 8 + rc) * pw + (size_t)bx * 8) = o;
}

// ---- upsampling, colour conversion ----------------------------------------------------------------------------------------------
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ c, const DGeom& g, int x, int y) {
    if (g.hs == 1) return c[(size_t)y * g.cw + x];
    const int cx = x >> 1;
    if (g.vs == 1) {                                                 // h2v1
        const uint8_t* r = c + (size_t)y * g.cw;
        if (g.ccw <= 2) return r[cx];
        return (x & 1) ? (3 * r[cx] + r[min(cx + 1, g.ccw - 1)] + 2) >> 2 : (3 * r[cx] + r[max(cx - 1, 0)] + 1) >> 2;
    }
    const int cy = y >> 1;                                           // h2v2
    const uint8_t* r = c + (size_t)cy * g.cw;
    if (g.ccw <= 2) return r[cx];
    const uint8_t* q = c + (size_t)((y & 1) ? min(cy + 1, g.cch - 1) : max(cy - 1, 0)) * g.cw;
    const int nx = (x & 1) ? min(cx + 1, g.ccw - 1) : max(cx - 1, 0);
    const int s = 3 * r[cx] + q[cx], sn = 3 * r[nx] + q[nx];
    return (3 * s + sn + ((x & 1) ? 7 : 8)) >> 4;
}

__global__ __launch_bounds__(256) void jpegd_pixels_kernel(const uint8_t* __restrict__ planes, uint8_t* __restrict__ out, const DGeom g) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= g.W) return;
    const int Y = planes[(size_t)y * g.yw + x];
    uint8_t* o = out + (size_t)y * g.stride;
    if (g.ncomp == 1) {
        o[x] = (uint8_t)Y;
        return;
    }
    const uint8_t* pcb = planes + (size_t)g.yw * g.yh;
    const int cb = chroma_at(pcb, g, x, y) - 128, cr = chroma_at(pcb + (size_t)g.cw * g.ch, g, x, y) - 128;
    const int R = Y + ((91881 * cr + 32768) >> 16);
    const int G = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16);
    const int B = Y + ((116130 * cb + 32768) >> 16);
    o[3 * x] = (uint8_t)min(max(R, 0), 255);
    o[3 * x + 1] = (uint8_t)min(max(G, 0), 255);
    o[3 * x + 2] = (uint8_t)min(max(B, 0), 255);
}

bool params_ok(const st_jpeg_dec_params* p, int64_t nbytes, DGeom& g) {
    if (nbytes < 1 || nbytes > kMaxFileBytes) return false;
    if (p->restart_interval < 0 || p->restart_interval > 65535 || p->reserved != 0) return false;
    if (!make_geom(p->H, p->W, p->ncomp, p->hs, p->vs, p->scan_len, g)) return false;
    if (p->scan_off < 0 || (int64_t)p->scan_off + p->scan_len > nbytes) return false;
    for (int c = 0; c < p->ncomp; ++c) {
        if (p->tq[c] < 0 || p->tq[c] > 1 || p->td[c] < 0 || p->td[c] > 1 || p->ta[c] < 0 || p->ta[c] > 1) return false;
        const int64_t q = p->q_off[p->tq[c]], d = p->dc_off[p->td[c]], a = p->ac_off[p->ta[c]];
        if (q < 0 || q + 64 > nbytes || d < 0 || d + 16 > nbytes || a < 0 || a + 16 > nbytes) return false;
    }
    return true;
}

// what both paths' sync and write kernels are told alike: where the file's tables are, and the MCU's shape
template <class Args>
Args scan_args(const uint8_t* file, int64_t nbytes, const st_jpeg_dec_params* p, const DGeom& g) {
    Args a;
    a.file = file, a.nbytes = (uint32_t)nbytes, a.td_bits = 0, a.ta_bits = 0;
    for (int i = 0; i < 2; ++i) a.dc_off[i] = (uint32_t)nbytes, a.ac_off[i] = (uint32_t)nbytes;          // an unused table reads as empty
    for (int c = 0; c < 3; ++c) {
        const int cc = c < g.ncomp ? c : 0;
        const int td = p->td[cc], ta = p->ta[cc];
        a.td_bits |= (uint32_t)td << c, a.ta_bits |= (uint32_t)ta << c;
        a.dc_off[td] = (uint32_t)p->dc_off[td], a.ac_off[ta] = (uint32_t)p->ac_off[ta];
    }
    a.nb = g.nb, a.ny = g.ny;
    return a;
}

// with restart intervals: the plain layout (its stream, coefficients and planes are used), then the restart tables (RGeom)
size_t workspace_bytes(const DGeom& g, int32_t restart_interval) {
    return g.ws_bytes + (restart_interval > 0 ? make_rst_geom(g.scan_len, (uint32_t)g.mcu_rows * (uint32_t)g.mcu_cols, (uint32_t)restart_interval).bytes : 0);
}

}  // namespace

extern "C" int st_abi_jpeg_dec_params_size(void) { return (int)sizeof(st_jpeg_dec_params); }

extern "C" int st_jpeg_dec_workspace_bytes(int32_t H, int32_t W, int32_t ncomp, int32_t hs, int32_t vs, int64_t scan_len) {
    DGeom g;
    return make_geom(H, W, ncomp, hs, vs, scan_len, g) && g.ws_bytes <= 0x7fffffff ? (int)g.ws_bytes : 0;
}

extern "C" int st_jpeg_dec_workspace_bytes_ex(const st_jpeg_dec_params* p) {
    DGeom g;
    if (!p || p->restart_interval < 0 || p->restart_interval > 65535 || p->reserved != 0 || !make_geom(p->H, p->W, p->ncomp, p->hs, p->vs, p->scan_len, g)) return 0;
    const size_t n = workspace_bytes(g, p->restart_interval);
    return n <= 0x7fffffff ? (int)n : 0;
}

extern "C" int st_jpeg_decode_u8(const void* file_dev, int64_t nbytes, const st_jpeg_dec_params* params, void* out, int64_t row_stride, int32_t* status_dev,
                                 void* workspace, int64_t workspace_bytes, void* stream) {
    DGeom g;
    if (!file_dev || !params || !out || !status_dev || !workspace || !params_ok(params, nbytes, g)) return ST_EINVAL;
    const size_t need = ::workspace_bytes(g, params->restart_interval);
    if (need > 0x7fffffff) return ST_EINVAL;
    if (row_stride < (int64_t)g.W * g.ncomp || row_stride > 0x7fffffff || ((uintptr_t)workspace & 15) || workspace_bytes < (int64_t)need) return ST_EINVAL;
    g.stride = (int32_t)row_stride;
    hipStream_t st = (hipStream_t)stream;
    const uint8_t* file = (const uint8_t*)file_dev;
    char* ws = (char*)workspace;
    uint32_t* tot = (uint32_t*)ws;
    uint32_t* cnt = (uint32_t*)(ws + g.off_cnt);
    uint8_t* bytes = (uint8_t*)(ws + g.off_stream);
    uint32_t* state = (uint32_t*)(ws + g.off_state);
    uint32_t* bnd = (uint32_t*)(ws + g.off_bnd);
    uint32_t* flags = (uint32_t*)(ws + g.off_flags);
    int16_t* coef = (int16_t*)(ws + g.off_coef);
    uint8_t* planes = (uint8_t*)(ws + g.off_planes);
    const uint32_t cap = g.nwg * kSyncThreads;
    const uint32_t stream_words = (uint32_t)(align16((size_t)g.scan_len + kPad) / 4);      // what off_stream reserves
    uint32_t q_off[3] = {0, 0, 0};
    for (int c = 0; c < 3; ++c) q_off[c] = (uint32_t)params->q_off[params->tq[c < g.ncomp ? c : 0]];
    const uint8_t* scan = file + params->scan_off;
    const uint32_t* words = (const uint32_t*)bytes;
    const uint32_t nmcu = (uint32_t)g.mcu_rows * (uint32_t)g.mcu_cols;
    const uint32_t coef_vec = g.nblocks * 8u;                              // uint4 per block: 8
    const uint32_t zero_wgs = (coef_vec + 255) / 256 < 1024 ? (coef_vec + 255) / 256 : 1024;
    if (params->restart_interval > 0) {                                    // its tables lie behind the plain layout; the plain state, bnd and flags stay unused
        const uint32_t ri = (uint32_t)params->restart_interval;
        const RGeom rg = make_rst_geom(g.scan_len, nmcu, ri);
        char* rws = ws + g.ws_bytes;
        uint32_t* rtot = (uint32_t*)rws;
        uint32_t* ndrop = (uint32_t*)(rws + rg.off_drop);
        uint32_t* nmark = (uint32_t*)(rws + rg.off_nmark);
        uint32_t* mark_pos = (uint32_t*)(rws + rg.off_mark);
        uint32_t* start = (uint32_t*)(rws + rg.off_start);
        uint32_t* first = (uint32_t*)(rws + rg.off_first);
        uint32_t* rstate = (uint32_t*)(rws + rg.off_state);
        uint32_t* blk = (uint32_t*)(rws + rg.off_blk);
        uint32_t* rbnd = (uint32_t*)(rws + rg.off_bnd);
        uint32_t* rflags = (uint32_t*)(rws + rg.off_flags);
        RScanArgs a = scan_args<RScanArgs>(file, nbytes, params, g);
        a.nmcu = nmcu, a.ri = ri, a.nint = rg.nint;
        hipLaunchKernelGGL(jpegd_zero_kernel, dim3(zero_wgs), dim3(256), 0, st, (uint4*)coef, coef_vec);
        ST_CHECK_LAUNCH();
        hipLaunchKernelGGL(jpegr_count_kernel, dim3(rg.nchunks), dim3(256), 0, st, scan, g.scan_len, ndrop, nmark);
        ST_CHECK_LAUNCH();
        hipError_t e = st_jpeg_scan_u32(ndrop, rg.nchunks, rtot, st);
        if (e != hipSuccess) return (int)e;
        e = st_jpeg_scan_u32(nmark, rg.nchunks, rtot + 1, st);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(jpegr_unstuff_kernel, dim3(rg.nchunks), dim3(256), 0, st, scan, g.scan_len, (const uint32_t*)ndrop, (const uint32_t*)nmark, (const uint32_t*)rtot, bytes,
                           mark_pos, rg.nint);
        ST_CHECK_LAUNCH();
        hipLaunchKernelGGL(jpegr_cut_kernel, dim3((rg.nint + 255) / 256), dim3(256), 0, st, (const uint32_t*)mark_pos, (const uint32_t*)rtot, g.scan_len, rg.nint, start, first,
                           status_dev);
        ST_CHECK_LAUNCH();
        e = st_jpeg_scan_u32(first, rg.nint, first + rg.nint, st);
        if (e != hipSuccess) return (int)e;
        for (uint32_t r = 0; r < rg.nwg; ++r) {
            hipLaunchKernelGGL(jpegr_sync_kernel, dim3(rg.nwg), dim3(kSyncThreads), 0, st, a, words, stream_words, (const uint32_t*)start, (const uint32_t*)first, rstate, rg.cap,
                               blk, rbnd, rflags, r, rg.nwg);
            ST_CHECK_LAUNCH();
        }
        e = st_jpeg_scan_u32(blk, rg.cap, blk + rg.cap, st);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(jpegr_write_kernel, dim3(rg.nwg), dim3(kSyncThreads), 0, st, a, words, stream_words, (const uint32_t*)start, (const uint32_t*)first,
                           (const uint32_t*)rstate, rg.cap, (const uint32_t*)blk, coef, status_dev);
        ST_CHECK_LAUNCH();
        hipLaunchKernelGGL(jpegr_dc_kernel, dim3(g.nb > 1 ? 3 : 1), dim3(1024), 0, st, coef, nmcu, g.nb, g.ny, ri);
        ST_CHECK_LAUNCH();
    } else {
        DScanArgs a = scan_args<DScanArgs>(file, nbytes, params, g);
        a.scan_len = g.scan_len, a.nblocks = g.nblocks;
        hipLaunchKernelGGL(jpegd_count_kernel, dim3(g.nchunks), dim3(256), 0, st, scan, g.scan_len, cnt);
        ST_CHECK_LAUNCH();
        hipError_t e = st_jpeg_scan_u32(cnt, g.nchunks, tot, st);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(jpegd_unstuff_kernel, dim3(g.nchunks), dim3(256), 0, st, scan, g.scan_len, (const uint32_t*)cnt, (const uint32_t*)tot, bytes);
        ST_CHECK_LAUNCH();
        for (uint32_t r = 0; r < g.nwg; ++r) {
            hipLaunchKernelGGL(jpegd_sync_kernel, dim3(g.nwg), dim3(kSyncThreads), 0, st, a, words, stream_words, (const uint32_t*)tot, state, cap, bnd, flags,
                               r, g.nwg);
            ST_CHECK_LAUNCH();
        }
        e = st_jpeg_scan_u32(state + 4 * (size_t)cap, cap, tot + 1, st);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(jpegd_zero_kernel, dim3(zero_wgs), dim3(256), 0, st, (uint4*)coef, coef_vec);
        ST_CHECK_LAUNCH();
        hipLaunchKernelGGL(jpegd_write_kernel, dim3(g.nwg), dim3(kSyncThreads), 0, st, a, words, stream_words, (const uint32_t*)tot, (const uint32_t*)state, cap,
                           coef, status_dev);
        ST_CHECK_LAUNCH();
        hipLaunchKernelGGL(jpegd_dc_kernel, dim3(g.ncomp), dim3(1024), 0, st, coef, nmcu, g.nb, g.ny);
        ST_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(jpegd_idct_kernel, dim3((g.nblocks + 31) / 32), dim3(256), 0, st, (const int16_t*)coef, file, q_off[0], q_off[1], q_off[2], planes, g);
    ST_CHECK_LAUNCH();
    hipLaunchKernelGGL(jpegd_pixels_kernel, dim3((g.W + 255) / 256, g.H), dim3(256), 0, st, (const uint8_t*)planes, (uint8_t*)out, g);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

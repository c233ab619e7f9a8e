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
// A file with restart intervals (st_jpeg_dec_params.restart_interval > 0) takes the zero, IDCT and pixel kernels from here; everything between
// the file's bytes and the DC-predicted coefficients is csrc/jpeg_rst.hip's (st_jpeg_rst_entropy, csrc/jpeg_rst.h).
#include "common.h"
#include "jpeg_dec_core.h"
#include "jpeg_scan.h"
#include "jpeg_rst.h"
#include "../../include/stitch_gfx950.h"

namespace {

constexpr int kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                              35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
struct NatTable {
    uint8_t v[64];
};
constexpr NatTable make_nat() {
    NatTable t{};
    for (int i = 0; i < 64; ++i) t.v[i] = (uint8_t)kNatural[i];
    return t;
}
__device__ const NatTable g_nat = make_nat();

constexpr int64_t kMaxPixels = (int64_t)1 << 24;
constexpr int64_t kMaxFileBytes = (int64_t)1 << 28;      // bit positions stay below 2^31
constexpr uint32_t kChunk = 2048;                        // scan bytes per workgroup of the unstuffing passes (256 threads x 8 bytes)
constexpr uint32_t kSubBits = 1024;                      // bits per subsequence (one thread)
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

// ---- unstuffing -----------------------------------------------------------------------------------------------------------------
// the 8 scan bytes from i0 and the byte before them; bit k of the result: byte i0 + k is a stuffed 0x00
__device__ __forceinline__ uint32_t stuffed_mask(const uint8_t* __restrict__ scan, uint32_t i0, uint32_t n, uint8_t (&b)[8]) {
    uint32_t prev = (i0 > 0 && i0 <= n) ? scan[i0 - 1] : 0u, m = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        b[k] = i0 + k < n ? scan[i0 + k] : (uint8_t)1;
        if (i0 + k < n && b[k] == 0 && prev == 255u) m |= 1u << k;
        prev = b[k];
    }
    return m;
}

__global__ __launch_bounds__(256) void jpegd_count_kernel(const uint8_t* __restrict__ scan, uint32_t n, uint32_t* __restrict__ cnt) {
    __shared__ uint32_t s_wave[4];
    uint8_t b[8];
    uint32_t ex;
    const uint32_t all = block_sum_256(__popc(stuffed_mask(scan, blockIdx.x * kChunk + threadIdx.x * 8, n, b)), ex, s_wave);
    if (threadIdx.x == 0) cnt[blockIdx.x] = all;
}

__global__ __launch_bounds__(256) void jpegd_unstuff_kernel(const uint8_t* __restrict__ scan, uint32_t n, const uint32_t* __restrict__ cnt_off,
                                                            const uint32_t* __restrict__ tot, uint8_t* __restrict__ dst) {
    __shared__ uint32_t s_wave[4];
    uint8_t b[8];
    const uint32_t i0 = blockIdx.x * kChunk + threadIdx.x * 8;
    const uint32_t m = stuffed_mask(scan, i0, n, b);
    uint32_t ex;
    block_sum_256(__popc(m), ex, s_wave);
    if (i0 < n) {
        uint8_t* o = dst + (i0 - cnt_off[blockIdx.x] - ex);
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (i0 + k < n && !((m >> k) & 1u)) *o++ = b[k];
    }
    if (blockIdx.x == 0 && threadIdx.x < kPad) dst[n - tot[0] + threadIdx.x] = 0;
}

// ---- entropy decoding -----------------------------------------------------------------------------------------------------------
struct DScanArgs {
    const uint8_t* file;
    uint32_t nbytes;
    uint32_t dc_off[2], ac_off[2];
    uint32_t nb, ny, td_bits, ta_bits;
    uint32_t scan_len, nblocks;
};

constexpr uint32_t kDhtBytes = 16 + 256;       // a DHT payload: the code counts, then at most 256 values

// the four DHT payloads come into LDS with one coalesced pass (bytes past the end of the file read as 0), then four threads build the
// decode tables from there: built straight from global memory, the ~300 dependent byte loads per table cost 0.2 ms per launch
__device__ __forceinline__ void load_tables(JdTables& t, uint8_t (&raw)[4][kDhtBytes], const DScanArgs& a) {
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
constexpr uint32_t kWgLds = kWgWords + 4;                        // + the two words a symbol that starts in the last bit reaches into (16-byte multiple)

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

// (a kernel, not a memset: every entry point of the library may be captured into a graph)
__global__ __launch_bounds__(256) void jpegd_zero_kernel(uint4* __restrict__ dst, uint32_t n) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) dst[i] = make_uint4(0u, 0u, 0u, 0u);
}

struct CoefSink {
    int16_t* coef;
    uint32_t nblocks;
    __device__ __forceinline__ void operator()(uint32_t block, uint32_t k, int v) const {
        if (block < nblocks) coef[(size_t)block * 64 + g_nat.v[k & 63u]] = (int16_t)v;
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

// ---- DC prediction --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void jpegd_dc_kernel(int16_t* __restrict__ coef, uint32_t nmcu, uint32_t nb, uint32_t ny) {
    __shared__ int s_wave[16];
    __shared__ int s_carry;
    const uint32_t c = blockIdx.x;
    const uint32_t n = c == 0 ? nmcu * ny : nmcu;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < n; base += 1024) {
        const uint32_t j = base + threadIdx.x;
        const size_t b = c == 0 ? (size_t)(j / ny) * nb + j % ny : (size_t)j * nb + ny + c - 1;
        const int v = j < n ? (int)coef[b * 64] : 0;
        int inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(inc, o, 64);
            if (lane >= o) inc += up;
        }
        if (lane == 63) s_wave[wv] = inc;
        __syncthreads();
        int before = s_carry;
        for (int k = 0; k < wv; ++k) before += s_wave[k];
        if (j < n) coef[b * 64] = (int16_t)(before + inc);
        __syncthreads();
        if (threadIdx.x == 1023) s_carry = before + inc;
        __syncthreads();
    }
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

// with restart intervals: the plain layout (its stream, coefficients and planes are used), then the tables of csrc/jpeg_rst.hip
size_t workspace_bytes(const DGeom& g, int32_t restart_interval) {
    return g.ws_bytes + (restart_interval > 0 ? st_jpeg_rst_workspace_bytes(g.scan_len, (uint32_t)g.mcu_rows * (uint32_t)g.mcu_cols, (uint32_t)restart_interval) : 0);
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
    DScanArgs a;
    a.file = file, a.nbytes = (uint32_t)nbytes, a.td_bits = 0, a.ta_bits = 0;
    for (int i = 0; i < 2; ++i) a.dc_off[i] = (uint32_t)nbytes, a.ac_off[i] = (uint32_t)nbytes;          // an unused table reads as empty
    uint32_t q_off[3] = {0, 0, 0};
    for (int c = 0; c < 3; ++c) {
        const int cc = c < g.ncomp ? c : 0;
        const int td = params->td[cc], ta = params->ta[cc];
        a.td_bits |= (uint32_t)td << c, a.ta_bits |= (uint32_t)ta << c;
        a.dc_off[td] = (uint32_t)params->dc_off[td], a.ac_off[ta] = (uint32_t)params->ac_off[ta];
        q_off[c] = (uint32_t)params->q_off[params->tq[cc]];
    }
    a.nb = g.nb, a.ny = g.ny, a.scan_len = g.scan_len, a.nblocks = g.nblocks;
    const uint8_t* scan = file + params->scan_off;
    const uint32_t coef_vec = g.nblocks * 8u;                              // uint4 per block: 8
    const uint32_t zero_wgs = (coef_vec + 255) / 256 < 1024 ? (coef_vec + 255) / 256 : 1024;
    if (params->restart_interval > 0) {                                    // the entropy decode of csrc/jpeg_rst.hip, behind the plain layout
        hipLaunchKernelGGL(jpegd_zero_kernel, dim3(zero_wgs), dim3(256), 0, st, (uint4*)coef, coef_vec);
        ST_CHECK_LAUNCH();
        JpegRstDecode d;
        d.file = file, d.nbytes = a.nbytes;
        for (int i = 0; i < 2; ++i) d.dc_off[i] = a.dc_off[i], d.ac_off[i] = a.ac_off[i];
        d.nb = g.nb, d.ny = g.ny, d.td_bits = a.td_bits, d.ta_bits = a.ta_bits;
        d.scan_off = (uint32_t)params->scan_off, d.scan_len = g.scan_len;
        d.nmcu = (uint32_t)g.mcu_rows * (uint32_t)g.mcu_cols, d.ri = (uint32_t)params->restart_interval;
        d.stream = bytes, d.stream_words = stream_words;
        d.coef = coef, d.status = status_dev, d.ws = ws + g.ws_bytes, d.st = st;
        const int rc = st_jpeg_rst_entropy(d);
        if (rc != ST_OK) return rc;
    } else {
        hipLaunchKernelGGL(jpegd_count_kernel, dim3(g.nchunks), dim3(256), 0, st, scan, g.scan_len, cnt);
        ST_CHECK_LAUNCH();
        hipError_t e = st_jpeg_scan_u32(cnt, g.nchunks, tot, st);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(jpegd_unstuff_kernel, dim3(g.nchunks), dim3(256), 0, st, scan, g.scan_len, (const uint32_t*)cnt, (const uint32_t*)tot, bytes);
        ST_CHECK_LAUNCH();
        for (uint32_t r = 0; r < g.nwg; ++r) {
            hipLaunchKernelGGL(jpegd_sync_kernel, dim3(g.nwg), dim3(kSyncThreads), 0, st, a, (const uint32_t*)bytes, stream_words, (const uint32_t*)tot, state, cap, bnd, flags,
                               r, g.nwg);
            ST_CHECK_LAUNCH();
        }
        e = st_jpeg_scan_u32(state + 4 * (size_t)cap, cap, tot + 1, st);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(jpegd_zero_kernel, dim3(zero_wgs), dim3(256), 0, st, (uint4*)coef, coef_vec);
        ST_CHECK_LAUNCH();
        hipLaunchKernelGGL(jpegd_write_kernel, dim3(g.nwg), dim3(kSyncThreads), 0, st, a, (const uint32_t*)bytes, stream_words, (const uint32_t*)tot, (const uint32_t*)state, cap,
                           coef, status_dev);
        ST_CHECK_LAUNCH();
        hipLaunchKernelGGL(jpegd_dc_kernel, dim3(g.ncomp), dim3(1024), 0, st, coef, (uint32_t)g.mcu_rows * (uint32_t)g.mcu_cols, g.nb, g.ny);
        ST_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(jpegd_idct_kernel, dim3((g.nblocks + 31) / 32), dim3(256), 0, st, (const int16_t*)coef, file, q_off[0], q_off[1], q_off[2], planes, g);
    ST_CHECK_LAUNCH();
    hipLaunchKernelGGL(jpegd_pixels_kernel, dim3((g.W + 255) / 256, g.H), dim3(256), 0, st, (const uint8_t*)planes, (uint8_t*)out, g);
    ST_CHECK_LAUNCH();
    return ST_OK;
}

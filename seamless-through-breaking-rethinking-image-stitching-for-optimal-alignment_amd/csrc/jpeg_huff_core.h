// libjpeg's jpeg_gen_optimal_table (jchuff.c) for csrc/jpeg.hip's table kernel, in plain C++ so that a host program
// (tools/jpeg_huff_host_check.cpp, built with the host compiler's sanitizers) runs exactly what the kernel runs.  Contract: README.md; CPU
// restatement: tests/_jpeg_opts_ref.py `gen_optimal_table`.
//
// The code is written for a team of W::LANES lanes that call it together (the kernel: one wave, LANES = 64; the host: LANES = 1).  Entry i of
// the 257 (256 symbols + the pseudo-symbol 256 of weight 1, which keeps the all-ones code free) belongs to lane i % LANES and lives in that
// lane's registers; W supplies `lane()`, `min2_u64(a, b)` (the lanes' two smallest keys a < b -> the team's two smallest, in every lane) and
// `sync()` (orders the team's accesses to JhWork).
//
//   jh_code_sizes   the merge loop: at most 256 rounds, each picks the two least frequent entries (among equals the LARGER index: the key is
//                   frequency << 9 | 256 - index) with one team-wide reduction of (smallest, second smallest).  libjpeg walks its `others`
//                   chains to make every code of the two trees one bit longer; here every entry carries the index of its tree's root
//                   instead, which reaches the same entries.
//   jh_finish       lane 0: counts per length, `huffval` (ordered by the length BEFORE limiting, then by symbol), the Annex K.2 adjustment to
//                   16 bits, the pseudo-symbol taken from the longest length
//   jh_assign_codes the canonical codes (Annex C), one symbol of `huffval` per lane and step
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define JH_HD __host__ __device__ __forceinline__
#else
#define JH_HD inline
#endif

constexpr int kJhEntries = 257;
constexpr int kJhMaxLen = 32;            // libjpeg's MAX_CLEN: it refuses an image whose unlimited code would be longer (more than 2^22 symbols
                                         // with Fibonacci-like counts); here such lengths count as 32, the file is then unspecified

struct JhWork {                          // the team's shared memory (the kernel: LDS)
    uint8_t codesize[kJhEntries];
    int32_t bits[kJhMaxLen + 1];         // [l]: codes of length l
    int32_t start[kJhMaxLen + 1];
    int32_t nsym;
    uint8_t huffval[256];
    uint32_t code[256];                  // by symbol: code | length << 16; 0: the symbol does not occur
};

template <class W>
JH_HD void jh_code_sizes(const W& w, const uint32_t* freq, JhWork& s) {
    constexpr int PER = (kJhEntries + W::LANES - 1) / W::LANES;
    constexpr uint64_t NONE = ~(uint64_t)0;
    const int lane = w.lane();
    uint32_t f[PER];
    int32_t root[PER], size[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int i = lane + k * W::LANES;
        f[k] = i < 256 ? freq[i] : (i == 256 ? 1u : 0u);
        root[k] = i, size[k] = 0;
    }
    for (;;) {
        uint64_t k1 = NONE, k2 = NONE;                              // the lane's two smallest keys (keys are distinct: they hold the index)
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const uint64_t key = f[k] ? ((uint64_t)f[k] << 9) | (uint32_t)(256 - (lane + k * W::LANES)) : NONE;
            if (key < k1) k2 = k1, k1 = key;
            else if (key < k2) k2 = key;
        }
        w.min2_u64(k1, k2);
        if (k2 == NONE) break;                                      // one entry left: the tree is complete
        const int c1 = 256 - (int)(k1 & 511u);
        const int c2 = 256 - (int)(k2 & 511u);
        const uint32_t sum = (uint32_t)(k1 >> 9) + (uint32_t)(k2 >> 9);
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int i = lane + k * W::LANES;
            if (i == c1) f[k] = sum;
            if (i == c2) f[k] = 0u;
            if (root[k] == c1 || root[k] == c2) root[k] = c1, ++size[k];
        }
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int i = lane + k * W::LANES;
        if (i < kJhEntries) s.codesize[i] = (uint8_t)(size[k] > kJhMaxLen ? kJhMaxLen : size[k]);
        if (i < 256) s.code[i] = 0u;
    }
    w.sync();
}

template <class W>
JH_HD void jh_finish(const W& w, JhWork& s) {
    if (w.lane() == 0) {
        for (int l = 0; l <= kJhMaxLen; ++l) s.bits[l] = 0;
        for (int i = 0; i < kJhEntries; ++i)
            if (s.codesize[i]) ++s.bits[s.codesize[i]];
        int32_t p = 0;
        for (int l = 1; l <= kJhMaxLen; ++l) {
            s.start[l] = p;
            p += s.bits[l] - (s.codesize[256] == l ? 1 : 0);
        }
        s.nsym = p;
        for (int j = 0; j < 256; ++j) {
            const int l = s.codesize[j];
            if (l) s.huffval[s.start[l]++] = (uint8_t)j;
        }
        for (int i = kJhMaxLen; i > 16; --i) {
            while (s.bits[i] > 0) {
                int j = i - 2;
                while (s.bits[j] == 0) --j;
                s.bits[i] -= 2, s.bits[i - 1] += 1, s.bits[j + 1] += 2, s.bits[j] -= 1;
            }
        }
        int i = 16;
        while (i > 0 && s.bits[i] == 0) --i;
        if (i > 0) --s.bits[i];
    }
    w.sync();
}

template <class W>
JH_HD void jh_assign_codes(const W& w, JhWork& s) {
    for (int k = w.lane(); k < s.nsym; k += W::LANES) {
        uint32_t code = 0;
        int32_t before = 0;
        for (int l = 1; l <= 16; ++l) {
            const int32_t n = s.bits[l];
            if (k < before + n) {
                s.code[s.huffval[k]] = (code + (uint32_t)(k - before)) | ((uint32_t)l << 16);
                break;
            }
            before += n;
            code = (code + (uint32_t)n) << 1;
        }
    }
    w.sync();
}

template <class W>
JH_HD void jh_gen_optimal_table(const W& w, const uint32_t* freq, JhWork& s) {
    jh_code_sizes(w, freq, s);
    jh_finish(w, s);
    jh_assign_codes(w, s);
}

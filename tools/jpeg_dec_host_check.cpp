// Runs the entropy decoder of csrc/jpeg_dec.hip (csrc/jpeg_dec_core.h, plain C++) on the host, stand-alone, so that the host compiler's
// sanitizers see it:   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I <pkg>/csrc tools/jpeg_dec_host_check.cpp
//
//   jpeg_dec_host_check <cases.bin> <out.bin>
//
// cases.bin: uint32 count, then per case: uint32 nbytes, the 15 int32 of `Case` below (what the host passes to the kernels), the file's
// bytes.  Per case the program unstuffs the scan as the kernels do, builds the four code tables from the file's
// bytes, decodes sequentially into int16 [nblocks, 64] (zigzag order, DC differences), and repeats the decode with the kernels' scheme:
// subsequences of 1024 bits from guessed states, rounds `start[i] <- end[i - 1]` to the fixpoint, a second pass that writes.  Both must
// give the same states, block counts and coefficients (exit status 2 otherwise).  out.bin: per case uint32 blocks found, then the
// coefficients.  tests/test_jpeg_dec_cpu.py feeds it the golden files, cut files and random bytes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpeg_dec_core.h"

struct Case {
    int32_t nblocks, nb, ny;
    int32_t td[3], ta[3];
    int32_t dc_off[2], ac_off[2];
    int32_t scan_off, scan_len;
};

struct VecSink {
    int16_t* coef;
    uint32_t nblocks;
    void operator()(uint32_t block, uint32_t k, int v) const {
        if (block < nblocks) coef[(size_t)block * 64 + (k & 63u)] = (int16_t)v;
    }
};

static const uint32_t kSubBits = 1024;

static bool same(const JdState& a, const JdState& b) { return a.pos == b.pos && a.slot == b.slot && a.k == b.k; }

int main(int argc, char** argv) {
    if (argc != 3) return 64;
    FILE* f = fopen(argv[1], "rb");
    FILE* o = fopen(argv[2], "wb");
    if (!f || !o) return 65;
    uint32_t count = 0;
    if (fread(&count, 4, 1, f) != 1) return 66;
    for (uint32_t ci = 0; ci < count; ++ci) {
        uint32_t nbytes = 0;
        Case c;
        if (fread(&nbytes, 4, 1, f) != 1 || fread(&c, sizeof(c), 1, f) != 1) return 66;
        std::vector<uint8_t> file(nbytes);                          // exactly nbytes: a read past the file is a heap overflow
        if (nbytes && fread(file.data(), 1, nbytes, f) != nbytes) return 66;
        // what st_jpeg_decode_u8 rejects before any launch never reaches the kernels
        if (c.scan_off < 0 || c.scan_len < 1 || (int64_t)c.scan_off + c.scan_len > (int64_t)nbytes || c.nb < 1 || c.ny < 1 || c.nblocks < 1) return 67;
        const uint8_t* scan = file.data() + c.scan_off;
        std::vector<uint8_t> un;
        for (int32_t j = 0; j < c.scan_len; ++j)
            if (!(j > 0 && scan[j] == 0 && scan[j - 1] == 0xFF)) un.push_back(scan[j]);
        const uint32_t n_un = (uint32_t)un.size();
        std::vector<uint32_t> words((n_un + 16 + 3) / 4, 0u);       // 16 zero bytes behind the stream, as the kernels leave them
        memcpy(words.data(), un.data(), n_un);
        JdTables t;
        for (int i = 0; i < 2; ++i) {
            jd_build_huff(t.dc[i], file.data(), nbytes, c.dc_off[i] < 0 ? nbytes : (uint32_t)c.dc_off[i]);
            jd_build_huff(t.ac[i], file.data(), nbytes, c.ac_off[i] < 0 ? nbytes : (uint32_t)c.ac_off[i]);
        }
        JdScan sc;
        sc.words = words.data(), sc.base_word = 0, sc.nbits = 8u * n_un, sc.nb = (uint32_t)c.nb, sc.ny = (uint32_t)c.ny;
        sc.td_bits = 0, sc.ta_bits = 0;
        for (int i = 0; i < 3; ++i) sc.td_bits |= ((uint32_t)c.td[i] & 1u) << i, sc.ta_bits |= ((uint32_t)c.ta[i] & 1u) << i;
        const uint32_t nblocks = (uint32_t)c.nblocks;
        std::vector<int16_t> seq((size_t)nblocks * 64, 0), par((size_t)nblocks * 64, 0);
        // sequential, one subsequence at a time so that the states at the cuts are known
        const uint32_t nsub = (sc.nbits + kSubBits - 1) / kSubBits > 0 ? (sc.nbits + kSubBits - 1) / kSubBits : 1;
        std::vector<JdState> want(nsub);
        std::vector<uint32_t> before(nsub);
        JdState st = {0, 0, 0};
        uint32_t total = 0;
        for (uint32_t i = 0; i < nsub; ++i) {
            want[i] = st, before[i] = total;
            total += jd_run(sc, t, st, (i + 1) * kSubBits, total, VecSink{seq.data(), nblocks});
        }
        // the kernels' scheme
        std::vector<JdState> start(nsub), end(nsub);
        std::vector<uint32_t> done(nsub);
        for (uint32_t i = 0; i < nsub; ++i) {
            start[i] = JdState{i * kSubBits, 0, 0};
            end[i] = start[i];
            done[i] = jd_run(sc, t, end[i], (i + 1) * kSubBits, 0, JdNoSink());
        }
        uint32_t rounds = 0;
        for (;; ++rounds) {
            if (rounds > nsub) return 2;                            // thread i is final after i rounds
            std::vector<uint32_t> changed;
            for (uint32_t i = 1; i < nsub; ++i)
                if (!same(start[i], end[i - 1])) changed.push_back(i);
            if (changed.empty()) break;
            for (uint32_t i : changed) start[i] = end[i - 1];
            for (uint32_t i : changed) {
                end[i] = start[i];
                done[i] = jd_run(sc, t, end[i], (i + 1) * kSubBits, 0, JdNoSink());
            }
        }
        uint32_t ptotal = 0;
        for (uint32_t i = 0; i < nsub; ++i) {
            if (!same(start[i], want[i]) || ptotal != before[i]) return 2;
            JdState s2 = start[i];
            ptotal += jd_run(sc, t, s2, (i + 1) * kSubBits, ptotal, VecSink{par.data(), nblocks});
        }
        if (ptotal != total || seq != par) return 2;
        fwrite(&total, 4, 1, o);
        fwrite(seq.data(), 2, seq.size(), o);
    }
    fclose(f);
    if (fclose(o)) return 65;
    return 0;
}

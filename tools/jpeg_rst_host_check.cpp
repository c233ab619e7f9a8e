// Runs the interval logic of csrc/jpeg_dec.hip's restart kernels (csrc/jpeg_rst_core.h and csrc/jpeg_dec_core.h, plain C++) on the host, stand-alone, so that the
// host compiler's sanitizers see it:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I <pkg>/csrc tools/jpeg_rst_host_check.cpp
//
//   jpeg_rst_host_check <cases.bin> <out.bin>
//
// cases.bin: uint32 count, then per case: uint32 nbytes, the 16 int32 of `Case` below (what the host passes to the kernels), the file's
// bytes.  Per case the program compacts the scan as the kernels do -- stuffed zeros and restart markers dropped, the offset behind every
// marker kept --, builds the four code tables from the file's bytes and decodes every interval in one piece from its known start state into
// int16 [nblocks, 64] (zigzag order, DC differences against 0 at an interval's start).  Then it repeats the decode with the kernels' scheme:
// every interval cut into its own subsequences of 1024 bits, the first one final, the others from guessed states, rounds
// `start[j] <- end[j - 1]` inside the intervals to the fixpoint, a second pass that writes inside the interval's blocks.  Both must give the
// same coefficients and status (exit status 2 otherwise).  out.bin: per case uint32 status, then the coefficients.
// tests/test_jpeg_rst_cpu.py feeds it the golden files, cut files, files with an interval's bytes removed and random bytes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpeg_rst_core.h"

struct Case {
    int32_t nblocks, nb, ny;
    int32_t td[3], ta[3];
    int32_t dc_off[2], ac_off[2];
    int32_t scan_off, scan_len;
    int32_t ri;
};

struct VecSink {
    int16_t* coef;
    uint32_t blk_end;
    void operator()(uint32_t block, uint32_t k, int v) const {
        if (block < blk_end) coef[(size_t)block * 64 + (k & 63u)] = (int16_t)v;
    }
};

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
        if (c.scan_off < 0 || c.scan_len < 1 || (int64_t)c.scan_off + c.scan_len > (int64_t)nbytes || c.nb < 1 || c.ny < 1 || c.nblocks < 1 || c.nblocks % c.nb ||
            c.ri < 1 || c.ri > 65535)
            return 67;
        const uint32_t nb = (uint32_t)c.nb, nmcu = (uint32_t)c.nblocks / nb, ri = (uint32_t)c.ri, nint = (nmcu + ri - 1) / ri;
        const uint8_t* scan = file.data() + c.scan_off;
        const uint32_t n = (uint32_t)c.scan_len;
        // jpegr_count_kernel / jpegr_unstuff_kernel, one byte at a time with the kernels' rule for a byte (jr_byte_class)
        std::vector<uint8_t> un;
        std::vector<uint32_t> mark(nint + 1, 0xDEADBEEFu);          // what a reused workspace may hold
        uint32_t found = 0;
        for (uint32_t j = 0; j < n; ++j) {
            const uint32_t prev = j > 0 ? scan[j - 1] : 0u, next = j + 1 < n ? scan[j + 1] : 0u;
            const uint32_t cls = jr_byte_class(prev, scan[j], next);
            if (!(cls & 1u)) un.push_back(scan[j]);
            if (cls & 2u) {
                ++found;
                if (found < nint) mark[found] = (uint32_t)un.size();
            }
        }
        const uint32_t n_un = (uint32_t)un.size();
        std::vector<uint32_t> words((n_un + 16 + 3) / 4, 0u);       // 16 zero bytes behind the stream, as the kernels leave them
        if (n_un) memcpy(words.data(), un.data(), n_un);
        // jpegr_cut_kernel and the prefix sum
        std::vector<uint32_t> start(nint + 1), first(nint + 1);
        for (uint32_t i = 0; i < nint; ++i) start[i] = jr_start(mark.data(), i, found, n_un);
        start[nint] = n_un;
        uint32_t nsub = 0;
        for (uint32_t i = 0; i < nint; ++i) first[i] = nsub, nsub += jr_nsub(start[i + 1] - start[i]);
        first[nint] = nsub;
        if (nsub > ((uint64_t)n * 8 + kJrSubBits - 1) / kJrSubBits + nint) return 2;       // the host's bound on the state arrays
        JdTables t;
        for (int i = 0; i < 2; ++i) {
            jd_build_huff(t.dc[i], file.data(), nbytes, c.dc_off[i] < 0 ? nbytes : (uint32_t)c.dc_off[i]);
            jd_build_huff(t.ac[i], file.data(), nbytes, c.ac_off[i] < 0 ? nbytes : (uint32_t)c.ac_off[i]);
        }
        JdScan sc;
        sc.words = words.data(), sc.base_word = 0, sc.nbits = 0, sc.nb = nb, sc.ny = (uint32_t)c.ny;
        sc.td_bits = 0, sc.ta_bits = 0;
        for (int i = 0; i < 3; ++i) sc.td_bits |= ((uint32_t)c.td[i] & 1u) << i, sc.ta_bits |= ((uint32_t)c.ta[i] & 1u) << i;
        const uint32_t nblocks = (uint32_t)c.nblocks;
        std::vector<int16_t> seq((size_t)nblocks * 64, 0), par((size_t)nblocks * 64, 0);
        // every interval in one piece
        uint32_t status = 0;
        for (uint32_t i = 0; i < nint; ++i) {
            const JrSub s = jr_sub(start.data(), first.data(), nint, ri, nb, nmcu, first[i]);
            if (s.ivl != i || s.local != 0 || s.blk_end > nblocks || s.blk0 >= s.blk_end) return 2;
            sc.nbits = s.end;
            JdState st = {s.lo, 0, 0};
            const uint32_t got = jd_run(sc, t, st, s.end, s.blk0, VecSink{seq.data(), s.blk_end});
            if (got != s.blk_end - s.blk0) status |= got < s.blk_end - s.blk0 ? 1u : 2u;
        }
        // the kernels' scheme
        std::vector<JrSub> sub(nsub);
        std::vector<JdState> st0(nsub), end(nsub);
        std::vector<uint32_t> done(nsub);
        for (uint32_t j = 0; j < nsub; ++j) {
            sub[j] = jr_sub(start.data(), first.data(), nint, ri, nb, nmcu, j);
            if (sub[j].lo > sub[j].limit || sub[j].limit > sub[j].end || (j > 0 && sub[j].lo < sub[j - 1].limit) || sub[j].limit - sub[j].lo > kJrSubBits) return 2;
            st0[j] = JdState{sub[j].lo, 0, 0};
            end[j] = st0[j];
            sc.nbits = sub[j].end;
            done[j] = jd_run(sc, t, end[j], sub[j].limit, 0, JdNoSink());
        }
        for (uint32_t rounds = 0;; ++rounds) {
            if (rounds > nsub) return 2;                            // subsequence j of an interval is final after j rounds
            std::vector<uint32_t> changed;
            for (uint32_t j = 1; j < nsub; ++j)
                if (sub[j].local > 0 && !same(st0[j], end[j - 1])) changed.push_back(j);
            if (changed.empty()) break;
            for (uint32_t j : changed) st0[j] = end[j - 1];
            for (uint32_t j : changed) {
                end[j] = st0[j];
                sc.nbits = sub[j].end;
                done[j] = jd_run(sc, t, end[j], sub[j].limit, 0, JdNoSink());
            }
        }
        std::vector<uint32_t> before(nsub + 1, 0);
        for (uint32_t j = 0; j < nsub; ++j) before[j + 1] = before[j] + done[j];
        uint32_t pstatus = 0;
        for (uint32_t j = 0; j < nsub; ++j) {
            const JrSub& s = sub[j];
            const uint32_t b0 = before[first[s.ivl]];
            JdState s2 = st0[j];
            sc.nbits = s.end;
            jd_run(sc, t, s2, s.limit, s.blk0 + (before[j] - b0), VecSink{par.data(), s.blk_end});
            if (s.local == 0) {
                const uint32_t got = before[first[s.ivl + 1]] - b0, want = s.blk_end - s.blk0;
                if (got != want) pstatus |= got < want ? 1u : 2u;
            }
        }
        if (pstatus != status || seq != par) return 2;
        fwrite(&status, 4, 1, o);
        fwrite(seq.data(), 2, seq.size(), o);
    }
    fclose(f);
    if (fclose(o)) return 65;
    return 0;
}

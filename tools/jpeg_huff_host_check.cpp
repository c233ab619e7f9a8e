// Runs the table builder of csrc/jpeg.hip's table kernel (csrc/jpeg_huff_core.h, plain C++) on the host, stand-alone, so that the host
// compiler's sanitizers see it:   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I <pkg>/csrc tools/jpeg_huff_host_check.cpp
//
//   jpeg_huff_host_check <cases.bin> <out.bin>
//
// cases.bin: uint32 count, then per case 256 uint32 symbol counts.  Per case the program builds the table as a team of one lane and checks
// what every table must satisfy (exit status 2 otherwise): no code longer than 16 bits, as many symbols as nonzero counts, a Kraft sum
// below 1 (the all-ones code stays free), per-symbol codes that are the canonical codes of (bits, huffval), every symbol with a nonzero
// count coded and no other.  out.bin: per case the 16 counts per length, uint32 number of symbols, the 256 huffval bytes (zero behind the
// symbols), the 256 code | length << 16 words.  tests/test_jpeg_opts_cpu.py compares them with tests/_jpeg_opts_ref.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "jpeg_huff_core.h"

struct OneLane {
    static constexpr int LANES = 1;
    int lane() const { return 0; }
    void min2_u64(uint64_t&, uint64_t&) const {}
    void sync() const {}
};

int main(int argc, char** argv) {
    if (argc != 3) return 64;
    FILE* f = fopen(argv[1], "rb");
    FILE* o = fopen(argv[2], "wb");
    if (!f || !o) return 65;
    uint32_t count = 0;
    if (fread(&count, 4, 1, f) != 1) return 66;
    for (uint32_t ci = 0; ci < count; ++ci) {
        std::vector<uint32_t> freq(256);                               // exactly 256: a read of entry 256 is a heap overflow
        if (fread(freq.data(), 4, 256, f) != 256) return 66;
        std::unique_ptr<JhWork> s(new JhWork);                         // on the heap, uninitialised: the builder must set what it reads
        jh_gen_optimal_table(OneLane{}, freq.data(), *s);
        uint32_t present = 0, nsym = 0, kraft = 0;
        for (int i = 0; i < 256; ++i) present += freq[i] ? 1u : 0u;
        for (int l = 1; l <= kJhMaxLen; ++l) {
            if (s->bits[l] < 0 || (l > 16 && s->bits[l] != 0)) return 2;
            if (l <= 16) nsym += (uint32_t)s->bits[l], kraft += (uint32_t)s->bits[l] << (16 - l);
        }
        if (nsym != present || (uint32_t)s->nsym != nsym || kraft >= 65536u) return 2;
        uint32_t code = 0, k = 0, coded = 0;
        for (int l = 1; l <= 16; ++l) {
            for (int n = 0; n < s->bits[l]; ++n, ++k) {
                const uint8_t sym = s->huffval[k];
                if (!freq[sym] || s->code[sym] != (code | ((uint32_t)l << 16))) return 2;
                ++code;
            }
            code <<= 1;
        }
        for (int i = 0; i < 256; ++i) coded += s->code[i] ? 1u : 0u;
        if (coded != nsym) return 2;
        uint8_t bits[16], vals[256];
        for (int l = 1; l <= 16; ++l) bits[l - 1] = (uint8_t)s->bits[l];
        for (uint32_t i = 0; i < 256; ++i) vals[i] = i < nsym ? s->huffval[i] : (uint8_t)0;
        fwrite(bits, 1, 16, o);
        fwrite(&nsym, 4, 1, o);
        fwrite(vals, 1, 256, o);
        fwrite(s->code, 4, 256, o);
    }
    fclose(f);
    if (fclose(o)) return 65;
    return 0;
}

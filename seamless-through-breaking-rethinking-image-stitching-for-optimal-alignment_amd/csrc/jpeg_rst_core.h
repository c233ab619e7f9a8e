// How csrc/jpeg_dec.hip cuts a scan with restart intervals into subsequences, in plain C++ so that a host program
// (tools/jpeg_rst_host_check.cpp, built with the host compiler's sanitizers) runs exactly what the kernels run.  Contract: README.md
// "Restart intervals"; CPU restatement: tests/_jpeg_rst_ref.py.
//
// The stream is the unstuffed scan WITHOUT its restart markers; interval i is its bytes [start[i], start[i + 1]) (start[0] = 0,
// start[n] = the stream's length; an interval whose marker is missing is empty at the end).  Interval i has jr_nsub(its bytes) >= 1
// subsequences of 1024 bits, first[i] is the index of its first one (the exclusive prefix sum; first[n] = their number).  Its first
// subsequence starts from a known state -- the interval's bit 0, slot 0, DC next -- and nothing crosses from one interval to the next:
// a subsequence reads no symbol that starts at or behind its interval's end, and writes no block outside [blk0, blk_end).
#pragma once
#include "jpeg_dec_core.h"

constexpr uint32_t kJrSubBits = 1024;

struct JrSub {
    uint32_t ivl;             // the interval of the subsequence
    uint32_t local;           // its index within the interval; 0: the start state is known
    uint32_t lo, limit;       // the symbols that start in bits [lo, limit) are its own
    uint32_t end;             // the interval's last bit + 1: JdScan::nbits while this subsequence decodes
    uint32_t blk0, blk_end;   // the interval's blocks
};

// What a scan byte is, given the byte in front of it and the byte behind it (0 at the scan's ends): bit 0: it is not part of the stream -- a
// stuffed 0x00 behind a 0xFF, or the 0xFF or the 0xD0..0xD7 of a restart marker --, bit 1: it is a restart marker's second byte
JD_HD uint32_t jr_byte_class(uint32_t prev, uint32_t cur, uint32_t next) {
    const bool rst = prev == 255u && (cur & 0xF8u) == 0xD0u;
    const bool drop = rst || (prev == 255u && cur == 0u) || (cur == 255u && (next & 0xF8u) == 0xD0u);
    return (drop ? 1u : 0u) | (rst ? 2u : 0u);
}

JD_HD uint32_t jr_nsub(uint32_t bytes) {
    const uint32_t n = (bytes * 8u + kJrSubBits - 1u) / kJrSubBits;             // bytes <= 2^28
    return n ? n : 1u;
}

// start of interval i: mark[i] is the stream offset behind the i-th marker (i = 1 .. found), a marker that was not found leaves its
// interval empty at the end of the stream
JD_HD uint32_t jr_start(const uint32_t* mark, uint32_t i, uint32_t found, uint32_t stream_bytes) {
    if (i == 0) return 0u;
    const uint32_t v = i <= found ? mark[i] : stream_bytes;
    return v < stream_bytes ? v : stream_bytes;
}

// the interval of subsequence j < first[n]: the last i with first[i] <= j (first is strictly increasing)
JD_HD uint32_t jr_find(const uint32_t* first, uint32_t n, uint32_t j) {
    uint32_t lo = 0, hi = n;                                                    // first[lo] <= j < first[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (first[mid] <= j) lo = mid;
        else hi = mid;
    }
    return lo;
}

// n intervals of ri MCUs (the last one: what is left of nmcu), nb blocks per MCU
JD_HD JrSub jr_sub(const uint32_t* start, const uint32_t* first, uint32_t n, uint32_t ri, uint32_t nb, uint32_t nmcu, uint32_t j) {
    JrSub s;
    s.ivl = jr_find(first, n, j);
    s.local = j - first[s.ivl];
    const uint32_t bit0 = start[s.ivl] * 8u;
    s.end = start[s.ivl + 1u] * 8u;
    s.lo = bit0 + s.local * kJrSubBits;
    s.limit = s.lo + kJrSubBits < s.end ? s.lo + kJrSubBits : s.end;
    const uint32_t m0 = s.ivl * ri, m1 = m0 + ri < nmcu ? m0 + ri : nmcu;       // n = ceil(nmcu / ri): m0 < nmcu
    s.blk0 = m0 * nb, s.blk_end = m1 * nb;
    return s;
}

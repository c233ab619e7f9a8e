// What csrc/jpeg_dec.hip hands to csrc/jpeg_rst.hip for a file with restart intervals: st_jpeg_decode_u8 checks the arguments, clears the
// coefficients, calls st_jpeg_rst_entropy for everything between the file's bytes and the DC-predicted coefficients, and goes on with its
// own IDCT and pixel kernels.
#pragma once
#include "common.h"

struct JpegRstDecode {
    const uint8_t* file;
    uint32_t nbytes;
    uint32_t dc_off[2], ac_off[2];       // DHT payloads in the file; nbytes: not defined
    uint32_t nb, ny, td_bits, ta_bits;   // blocks per MCU, of them luma; bit c: the DC / AC table of component c
    uint32_t scan_off, scan_len;
    uint32_t nmcu, ri;                   // MCUs of the frame, MCUs per restart interval (1..65535)
    uint8_t* stream;                     // room for the unstuffed stream: stream_words * 4 >= scan_len + 16 bytes, 16-byte aligned
    uint32_t stream_words;
    int16_t* coef;                       // [nmcu * nb, 64], zero
    int32_t* status;
    void* ws;                            // st_jpeg_rst_workspace_bytes, 16-byte aligned
    hipStream_t st;
};

size_t st_jpeg_rst_workspace_bytes(uint32_t scan_len, uint32_t nmcu, uint32_t ri);
int st_jpeg_rst_entropy(const JpegRstDecode& d);

// What csrc/jpeg.hip hands to csrc/jpeg_rst.hip for a file it writes with restart intervals (st_jpeg_enc_params.reserved[0] > 0): the block,
// table, zero, count and scan kernels stay csrc/jpeg.hip's, the steps below replace what differs.  `dev` is the JDev of csrc/jpeg_enc_core.h
// (nullptr: the Annex K tables), `header` its JHeader: both types have internal linkage, so they cross as untyped pointers.
struct JpegRstEncode {
    const int16_t* coef;                 // [nblocks, 64] zigzag order, absolute DC
    uint32_t* len;                       // [nblocks]: bits per block, then the bit offset of every block in the padded stream
    uint32_t* tot;                       // [0] bits of the padded stream, [1] its 0xFF bytes, [2] padding bits
    uint32_t* pad;                       // [nint + 1]: padding bits behind interval i, then their exclusive prefix sum
    uint32_t* ibyte;                     // [nint + 1]: the stream byte interval i starts at
    uint32_t* stream;
    uint32_t stream_words;
    void* dev;
    uint32_t nblocks, nb, ny;
    uint32_t ri, nint, nchunks;
    const uint32_t* cnt;                 // 0xFF bytes in front of every 2048-byte chunk of the stream
    uint8_t* out;
    int32_t* out_nbytes;
    const void* header;
    hipStream_t st;
};

int st_jpeg_rst_hist(const JpegRstEncode& e);        // the four histograms, DC differences against 0 at an interval's start
int st_jpeg_rst_offsets(const JpegRstEncode& e);     // bits per block -> bit offsets, every interval's end rounded up to a byte
int st_jpeg_rst_pack(const JpegRstEncode& e);        // the codes at their offsets, 1-bit padding behind every interval
int st_jpeg_rst_stuff(const JpegRstEncode& e);       // header with DRI, stuffed bytes, the markers between the intervals, EOI, byte count

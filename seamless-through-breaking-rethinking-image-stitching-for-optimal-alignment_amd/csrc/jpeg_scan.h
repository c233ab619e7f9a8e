// What the JPEG encoder (csrc/jpeg.hip) and decoder (csrc/jpeg_dec.hip) share: the prefix sum over a table of counts and the sum over a
// workgroup of 256 threads.
#pragma once
#include "common.h"

// in-place exclusive prefix sum of data[0 .. n), total -> *total: jpeg_scan_kernel of csrc/jpeg.hip, one workgroup
hipError_t st_jpeg_scan_u32(uint32_t* data, uint32_t n, uint32_t* total, hipStream_t st);

namespace {

// sum of v over the workgroup's 256 threads (4 waves; s_wave: 4 words of LDS), `exclusive`: the sum over the threads before this one
__device__ __forceinline__ uint32_t block_sum_256(uint32_t v, uint32_t& exclusive, uint32_t* s_wave) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    if (lane == 63) s_wave[wv] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (int k = 0; k < 4; ++k) {
        if (k < wv) before += s_wave[k];
        all += s_wave[k];
    }
    exclusive = before + inc - v;
    return all;
}

}  // namespace

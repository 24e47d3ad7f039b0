// Inline helpers that several objects of libglove_prep_hip.so use: the merge-path search, 16-B moves of 8-byte words between
// memory and LDS, a block scan, a device-side count, an overlap test.  No kernels: a kernel the objects share is compiled
// once, in glove_table_ops.hip, and reached through a host function (glove_table_ops.h).
#pragma once
#include "glove_common.h"
#include "glove_cooc_keys.h"      // kNoKey

namespace glove {

// How many of the first `diag` entries of the merged order (ties to A) come from A.
template <typename I>
__device__ inline I merge_path(const uint64_t *__restrict__ A, I na, const uint64_t *__restrict__ B, I nb, I diag)
{
    I lo = diag > nb ? diag - nb : 0, hi = diag < na ? diag : na;
    while (lo < hi) {
        const I mid = (lo + hi) >> 1;
        if (A[mid] <= B[diag - 1 - mid]) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ inline int64_t clamp_count(const int64_t *n, int64_t cap)
{
    const int64_t v = *n;
    return v < 0 ? 0 : (v > cap ? cap : v);
}

// n 8-byte words from g to LDS / from LDS to g: 16 B per lane from the first 16-B aligned word on
__device__ inline void load_words(const uint64_t *__restrict__ g, int n, uint64_t *s)
{
    const int head = (((uintptr_t)g & 15) != 0 && n > 0) ? 1 : 0;
    const int pairs = (n - head) >> 1;
    if (threadIdx.x == 0 && head) s[0] = g[0];
    const ulonglong2 *g2 = (const ulonglong2 *)(g + head);
    for (int p = threadIdx.x; p < pairs; p += kBlock) {
        const ulonglong2 v = g2[p];
        s[head + 2 * p] = v.x;
        s[head + 2 * p + 1] = v.y;
    }
    if (threadIdx.x == 0 && ((n - head) & 1)) s[n - 1] = g[n - 1];
}

__device__ inline void store_words(uint64_t *__restrict__ g, int n, const uint64_t *s)
{
    const int head = (((uintptr_t)g & 15) != 0 && n > 0) ? 1 : 0;
    const int pairs = (n - head) >> 1;
    if (threadIdx.x == 0 && head) g[0] = s[0];
    ulonglong2 *g2 = (ulonglong2 *)(g + head);
    for (int p = threadIdx.x; p < pairs; p += kBlock) {
        ulonglong2 v;
        v.x = s[head + 2 * p];
        v.y = s[head + 2 * p + 1];
        g2[p] = v;
    }
    if (threadIdx.x == 0 && ((n - head) & 1)) g[n - 1] = s[n - 1];
}

// block-wide exclusive scan of one int per thread (wave scan, then the wave totals): `before` = the sum over the threads
// in front, `total` = the block's sum.  s_wave: kBlock / 64 ints of LDS.  Holds a __syncthreads.
__device__ inline void block_exclusive_scan(int mine, int *s_wave, int &before, int &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = mine;
#pragma unroll
    for (int dlt = 1; dlt < 64; dlt <<= 1) {
        const int up = __shfl_up(incl, dlt, 64);
        if (lane >= dlt) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    before = incl - mine;
    total = 0;
#pragma unroll
    for (int wv = 0; wv < kBlock / 64; ++wv) {
        if (wv < wave) before += s_wave[wv];
        total += s_wave[wv];
    }
}

inline bool overlap(const void *p, size_t pn, const void *q, size_t qn)
{
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + qn && b < a + pn;
}

}  // namespace glove

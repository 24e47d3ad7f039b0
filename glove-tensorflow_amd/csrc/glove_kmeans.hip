// Spherical k-means over the rows of an embedding table on gfx950: the third object of libglove_eval_hip.so,
// include/glove_eval_cluster_hip.h (the semantics and the summation order are stated there).
//
//   glove_kmeans_assign_f32   every point's closest centroid by cosine: the similarity GEMM (glove_sim_gemm.h) with
//                             the arg-max kept inside it — no n x K score matrix exists.
//   glove_kmeans_update_f32   the new centroids, bitwise repeatable and without float atomics: a stable counting sort of
//                             the point indices by cluster, then chunked segmented sums in a fixed order.
//
// The inverse-norm kernels, the row helpers and the order topk_before come from glove_topk_kernels.h / glove_common.h.
#include "glove_common.h"
#include "glove_topk_kernels.h"
#include "../../include/glove_eval_cluster_hip.h"

namespace glove {

constexpr int kKmMaxK = 4096;
constexpr int kKmPoints = 128, kKmCents = 128;     // the assign workgroup's point tile / one centroid tile of its walk
constexpr int kKmTile = 2048;                      // points per tile of the counting sort
constexpr int kKmChunk = 64;                       // rows one lane group sums (the header states it: part of the bits)
constexpr int kKmLevels = 4;                       // 64^4 > 65535 * 128: four summation levels reduce any cluster to one row

// assign[i] = argmax_c (W[ids[i]] . C[c]) pinv[i] cinv[c] in the order topk_before, cos[i] the winner's score clamped.
// Workgroup = 128 points; it walks the centroids in tiles of 128 and runs, per tile, sim_tile_gemm (four waves of
// 2 x 2 blocks, as in cosine_mfma_kernel) with the CENTROIDS on the A side: in the C/D map a lane then holds 16
// centroid rows (per block) of ONE point column, so the running arg-max of a point stays in two registers of its
// lane.  At the end the two half-waves of a point's column exchange once, and the two waves that hold the two
// centroid halves of a tile meet through LDS.  A dot product is a k-ordered fma chain: its bits do not depend on the
// tile, the point's place in the call or n.
__global__ __launch_bounds__(kBlock) void kmeans_assign_kernel(const float *__restrict__ W, int32_t d,
                                                               const int32_t *__restrict__ ids, int32_t n,
                                                               const float *__restrict__ C, int32_t K,
                                                               const float *__restrict__ pinv,
                                                               const float *__restrict__ cinv,
                                                               int32_t *__restrict__ assign_out,
                                                               float *__restrict__ cos_out)
{
    __shared__ float Cs[kKmCents][kSimK + 1];
    __shared__ float Ps[kKmPoints][kSimK + 1];
    __shared__ int32_t p_id[kKmPoints];                    // the tile's points: -1 beyond n
    __shared__ float p_inv[kKmPoints];
    __shared__ float c_inv[kKmCents];
    __shared__ float red_s[kKmPoints];                     // the upper centroid half's winners, for the lower half's waves
    __shared__ int32_t red_c[kKmPoints];
    const int p0 = blockIdx.x * kKmPoints;
    if (threadIdx.x < kKmPoints) {
        const bool in = p0 + threadIdx.x < n;
        p_id[threadIdx.x] = in ? ids[p0 + threadIdx.x] : -1;
        p_inv[threadIdx.x] = in ? pinv[p0 + threadIdx.x] : 0.f;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;               // this wave's 64 centroids of a tile and 64 points
    const int r32 = lane & 31, kh = lane >> 5;
    float best[2] = {-INFINITY, -INFINITY};                // of point wn * 64 + b * 32 + r32, over this lane's centroid rows
    int32_t best_c[2] = {0x7fffffff, 0x7fffffff};

    for (int c0 = 0; c0 < K; c0 += kKmCents) {
        __syncthreads();                                   // the last tile's epilogue has read c_inv
        if (threadIdx.x < kKmCents) c_inv[threadIdx.x] = c0 + threadIdx.x < K ? cinv[c0 + threadIdx.x] : 0.f;
        f32x16 acc[2][2];
        sim_tile_gemm(Cs, Ps, acc, C, W, d, [&](int row) { return c0 + row < K ? c0 + row : -1; },
                      [&](int row) { return p_id[row]; }, wm * 64, 32, wn * 64);
        // C/D map: column = point, row = centroid
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const float pi = p_inv[wn * 64 + b * 32 + r32];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int cl = wm * 64 + a * 32 + sim_cd_row(reg, kh), c = c0 + cl;
                    const float s = acc[a][b][reg] * pi * c_inv[cl];
                    if (c < K && topk_before(s, c, best[b], best_c[b])) { best[b] = s; best_c[b] = c; }
                }
            }
        }
    }
#pragma unroll
    for (int b = 0; b < 2; ++b) {                          // the other half-wave holds the other 16 rows of each block
        const float os = __shfl_xor(best[b], 32, 64);
        const int32_t oc = __shfl_xor(best_c[b], 32, 64);
        if (topk_before(os, oc, best[b], best_c[b])) { best[b] = os; best_c[b] = oc; }
    }
    if (wm == 1 && kh == 0) {
#pragma unroll
        for (int b = 0; b < 2; ++b) { red_s[wn * 64 + b * 32 + r32] = best[b]; red_c[wn * 64 + b * 32 + r32] = best_c[b]; }
    }
    __syncthreads();
    if (wm == 0 && kh == 0) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int pl = wn * 64 + b * 32 + r32;
            if (topk_before(red_s[pl], red_c[pl], best[b], best_c[b])) { best[b] = red_s[pl]; best_c[b] = red_c[pl]; }
            if (p0 + pl < n) {
                const bool none = best_c[b] == 0x7fffffff;      // every score a NaN: the point goes to cluster 0
                assign_out[p0 + pl] = none ? 0 : best_c[b];
                cos_out[p0 + pl] = none ? 0.f : clamp_cos(best[b]);
            }
        }
    }
}

__device__ inline bool km_key_ok(int32_t key, int32_t K) { return (uint32_t)key < (uint32_t)K; }

// hist[tile, c] = members of cluster c among the tile's points (integer atomics in LDS: the result is order-free)
__global__ __launch_bounds__(kBlock) void kmeans_hist_kernel(const int32_t *__restrict__ assign, int32_t n, int32_t K,
                                                             int32_t *__restrict__ hist)
{
    __shared__ int32_t h[kKmMaxK];
    for (int c = threadIdx.x; c < K; c += kBlock) h[c] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kKmTile;
#pragma unroll
    for (int e = 0; e < kKmTile / kBlock; ++e) {
        const int64_t i = base + e * kBlock + threadIdx.x;
        if (i < n) {
            const int32_t key = assign[i];
            if (km_key_ok(key, K)) atomicAdd(&h[key], 1);
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < K; c += kBlock) hist[(size_t)blockIdx.x * K + c] = h[c];
}

// One thread per cluster walks the tiles: hist[tile, c] becomes the members of c in earlier tiles, counts[c] the size
// of c.  Sixteen loads are issued before the first is used.
__global__ __launch_bounds__(kBlock) void kmeans_colscan_kernel(int32_t *__restrict__ hist, int32_t ntiles, int32_t K,
                                                                int32_t *__restrict__ counts)
{
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= K) return;
    int32_t run = 0;
    for (int t0 = 0; t0 < ntiles; t0 += 16) {
        int32_t v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = t0 + j < ntiles ? hist[(size_t)(t0 + j) * K + c] : 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (t0 + j < ntiles) hist[(size_t)(t0 + j) * K + c] = run;
            run += v[j];
        }
    }
    counts[c] = run;
}

// starts[l, c], l = 0 .. kKmLevels: where cluster c's rows begin at summation level l — level 0 the sorted point
// indices, level l + 1 the sums of level l's chunks (m -> ceil(m / 64) rows per cluster); starts[l, K] is the level's
// total.  One workgroup: a thread owns 16 consecutive clusters, the 256 partial sums are scanned in LDS.
__global__ __launch_bounds__(kBlock) void kmeans_starts_kernel(const int32_t *__restrict__ counts, int32_t K,
                                                               int32_t *__restrict__ starts)
{
    __shared__ int32_t part[kBlock];
    constexpr int kOwn = kKmMaxK / kBlock;
    const int t = threadIdx.x;
    int32_t m[kOwn];
#pragma unroll
    for (int j = 0; j < kOwn; ++j) m[j] = t * kOwn + j < K ? counts[t * kOwn + j] : 0;
    for (int l = 0; l <= kKmLevels; ++l) {
        int32_t s = 0;
#pragma unroll
        for (int j = 0; j < kOwn; ++j) s += m[j];
        part[t] = s;
        __syncthreads();
        for (int off = 1; off < kBlock; off <<= 1) {
            const int32_t v = t >= off ? part[t - off] : 0;
            __syncthreads();
            part[t] += v;
            __syncthreads();
        }
        int32_t run = part[t] - s;
        int32_t *out = starts + (size_t)l * (K + 1);
#pragma unroll
        for (int j = 0; j < kOwn; ++j) {
            if (t * kOwn + j < K) out[t * kOwn + j] = run;
            run += m[j];
            m[j] = (m[j] + kKmChunk - 1) / kKmChunk;
        }
        if (t == kBlock - 1) out[K] = part[t];
        __syncthreads();
    }
}

// sorted[starts[0, c] + (members of c in earlier tiles) + (earlier members of c in this tile)] = i: the stable counting
// sort's scatter.  One wave per tile walks it 64 points at a time in ascending i; a point's rank among the 64 is the
// number of lower lanes with its key (digit_peers), and the lowest of them advances the cluster's counter in LDS.
__global__ __launch_bounds__(64) void kmeans_scatter_kernel(const int32_t *__restrict__ assign, int32_t n, int32_t K,
                                                            int key_bits, const int32_t *__restrict__ hist,
                                                            const int32_t *__restrict__ starts0,
                                                            int32_t *__restrict__ sorted)
{
    __shared__ int32_t next[kKmMaxK];
    const int lane = threadIdx.x;
    for (int c = lane; c < K; c += 64) next[c] = starts0[c] + hist[(size_t)blockIdx.x * K + c];
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kKmTile;
    for (int r = 0; r < kKmTile / 64; ++r) {
        const int64_t i = base + r * 64 + lane;
        int32_t key = i < n ? assign[i] : -1;
        const bool valid = km_key_ok(key, K);
        if (!valid) key = 0;
        const unsigned long long peers = digit_peers(key, key_bits, valid);
        const unsigned long long lower = peers & ((1ull << lane) - 1ull);
        const int32_t at = next[key];                      // every peer reads before the first of them writes
        __syncthreads();
        if (valid) {
            const int32_t pos = at + __popcll(lower);
            if (pos < n) sorted[pos] = (int32_t)i;          // (always, for an assign array that stands still during the call)
            if (lower == 0) next[key] = at + __popcll(peers);
        }
        __syncthreads();
    }
}

// One summation level: output row g = the sum of one chunk of at most 64 consecutive input rows of one cluster, in
// order, starting from the first.  FIRST: the input rows are the unit rows of the points sorted[...]; otherwise rows of
// `src`, the level before.  The lane group finds its cluster by bisection of the output level's starts.
template <int LPR, int NV, bool FIRST>
__global__ __launch_bounds__(kBlock) void kmeans_segsum_kernel(const float *__restrict__ W, int d4,
                                                               const int32_t *__restrict__ ids,
                                                               const int32_t *__restrict__ sorted,
                                                               const float *__restrict__ src,
                                                               const int32_t *__restrict__ st_in,
                                                               const int32_t *__restrict__ st_out, int32_t K,
                                                               float *__restrict__ dst)
{
    constexpr int GPB = kBlock / LPR;
    const int lg = threadIdx.x % LPR, grp = threadIdx.x / LPR;
    const int32_t total = st_out[K];
    for (int32_t g = blockIdx.x * GPB + grp; g < total; g += gridDim.x * GPB) {
        int lo = 0, hi = K;                                // st_out[lo] <= g < st_out[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (st_out[mid] <= g) lo = mid; else hi = mid;
        }
        const int32_t first = st_in[lo] + (g - st_out[lo]) * kKmChunk;
        int32_t cnt = st_in[lo + 1] - first;
        cnt = cnt < kKmChunk ? cnt : kKmChunk;
        f4 acc[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) acc[k] = f4{0.f, 0.f, 0.f, 0.f};
        for (int t = 0; t < cnt; ++t) {
            f4 r[NV];
            if constexpr (FIRST) {
                load_row_p<LPR, NV>(r, W, ids[sorted[first + t]], d4, lg);
                const float inv = clamped_inv_norm(row_sumsq<LPR, NV>(r));
#pragma unroll
                for (int k = 0; k < NV; ++k) r[k] *= inv;
            } else {
                load_row_p<LPR, NV>(r, src, first + t, d4, lg);
            }
#pragma unroll
            for (int k = 0; k < NV; ++k) acc[k] = t == 0 ? r[k] : acc[k] + r[k];
        }
        store_row_p<LPR, NV>(dst, g, d4, lg, acc);
    }
}

// C_out[c] = the cluster's one remaining row over its clamped norm; an empty cluster's row of C_in, bit for bit
template <int LPR, int NV>
__global__ __launch_bounds__(kBlock) void kmeans_finish_kernel(const float *__restrict__ sums,
                                                               const int32_t *__restrict__ st_last,
                                                               const int32_t *__restrict__ counts,
                                                               const float *__restrict__ C_in, int d4, int32_t K,
                                                               float *__restrict__ C_out)
{
    constexpr int GPB = kBlock / LPR;
    const int lg = threadIdx.x % LPR, grp = threadIdx.x / LPR;
    for (int c = blockIdx.x * GPB + grp; c < K; c += gridDim.x * GPB) {
        f4 r[NV];
        const bool empty = counts[c] == 0;
        if (empty) load_row_p<LPR, NV>(r, C_in, c, d4, lg);
        else load_row_p<LPR, NV>(r, sums, st_last[c], d4, lg);
        const float inv = clamped_inv_norm(row_sumsq<LPR, NV>(r));
        if (!empty) {
#pragma unroll
            for (int k = 0; k < NV; ++k) r[k] *= inv;
        }
        store_row_p<LPR, NV>(C_out, c, d4, lg, r);
    }
}

// the workspace (the header states it): every piece 256-B aligned
struct KmeansWs {
    float *pinv, *cinv;
    int32_t *hist, *starts, *sorted;
    float *sums[2];
    int32_t ntiles;
    int64_t rows[2];
    size_t bytes;
};

static KmeansWs carve_kmeans_ws(void *ws, int32_t n, int32_t d, int32_t K)
{
    WsCarver c{(char *)ws};
    KmeansWs s;
    s.ntiles = (n + kKmTile - 1) / kKmTile;
    s.rows[0] = (int64_t)n / kKmChunk + K;
    s.rows[1] = s.rows[0] / kKmChunk + K;
    s.pinv = c.take<float>((size_t)n);
    s.cinv = c.take<float>((size_t)K);
    s.hist = c.take<int32_t>((size_t)s.ntiles * K);
    s.starts = c.take<int32_t>((size_t)(kKmLevels + 1) * (K + 1));
    s.sorted = c.take<int32_t>((size_t)n);
    s.sums[0] = c.take<float>((size_t)s.rows[0] * d);
    s.sums[1] = c.take<float>((size_t)s.rows[1] * d);
    s.bytes = c.off;
    return s;
}

static bool kmeans_sizes_ok(int32_t n, int32_t V, int32_t d, int32_t K)
{
    return n >= 0 && n <= 65535 * 128 && K >= 1 && K <= kKmMaxK && sim_table_ok(V, d);
}

}  // namespace glove

using namespace glove;

extern "C" {

int glove_eval_cluster_abi_version(void) { return GLOVE_EVAL_CLUSTER_ABI_VERSION; }

size_t glove_kmeans_workspace_bytes(int32_t n, int32_t V, int32_t d, int32_t K)
{
    if (!kmeans_sizes_ok(n, V, d, K)) return 0;
    return carve_kmeans_ws(nullptr, n, d, K).bytes;
}

int glove_kmeans_assign_f32(const float *W, int32_t V, int32_t d, const int32_t *ids, int32_t n, const float *C, int32_t K,
                            int32_t *assign_out, float *cos_out, void *ws, size_t ws_bytes, void *stream)
{
    if (!kmeans_sizes_ok(n, V, d, K)) return GLOVE_E_BADARG;
    if (n == 0) return 0;
    if (!W || !ids || !C || !assign_out || !cos_out || !ws) return GLOVE_E_BADARG;
    const KmeansWs w = carve_kmeans_ws(ws, n, d, K);
    if (w.bytes > ws_bytes) return GLOVE_E_WORKSPACE;
    const int d4 = d / 4;
    const RowShape shape = pick_row_shape(d4);
    const int nbp = blocks_for(n, kBlock / shape.lpr), nbc = blocks_for(K, kBlock / shape.lpr);
    hipStream_t st = (hipStream_t)stream;
#define CALL(LPR, NV)                                                                                                  \
    hipLaunchKernelGGL((gathered_inv_norm_kernel<LPR, NV>), dim3(nbp), dim3(kBlock), 0, st, W, d4, ids, n, w.pinv);    \
    hipLaunchKernelGGL((inv_norm_kernel<LPR, NV>), dim3(nbc), dim3(kBlock), 0, st, C, K, d4, w.cinv)
    GLOVE_DISPATCH_ROW_SHAPE(shape, CALL);
#undef CALL
    hipLaunchKernelGGL(kmeans_assign_kernel, dim3((n + kKmPoints - 1) / kKmPoints), dim3(kBlock), 0, st, W, d, ids, n, C, K,
                       w.pinv, w.cinv, assign_out, cos_out);
    return (int)hipGetLastError();
}

int glove_kmeans_update_f32(const float *W, int32_t V, int32_t d, const int32_t *ids, int32_t n, const int32_t *assign,
                            const float *C_in, int32_t K, float *C_out, int32_t *counts_out, void *ws, size_t ws_bytes,
                            void *stream)
{
    if (!kmeans_sizes_ok(n, V, d, K)) return GLOVE_E_BADARG;
    if (n == 0) return 0;
    if (!W || !ids || !assign || !C_in || !C_out || !counts_out || !ws || C_out == C_in) return GLOVE_E_BADARG;
    const KmeansWs w = carve_kmeans_ws(ws, n, d, K);
    if (w.bytes > ws_bytes) return GLOVE_E_WORKSPACE;
    const int d4 = d / 4;
    const RowShape shape = pick_row_shape(d4);
    const int gpb = kBlock / shape.lpr;
    hipStream_t st = (hipStream_t)stream;
    int key_bits = 0;
    while ((1 << key_bits) < K) ++key_bits;
    hipLaunchKernelGGL(kmeans_hist_kernel, dim3(w.ntiles), dim3(kBlock), 0, st, assign, n, K, w.hist);
    hipLaunchKernelGGL(kmeans_colscan_kernel, dim3((K + kBlock - 1) / kBlock), dim3(kBlock), 0, st, w.hist, w.ntiles, K, counts_out);
    hipLaunchKernelGGL(kmeans_starts_kernel, dim3(1), dim3(kBlock), 0, st, counts_out, K, w.starts);
    hipLaunchKernelGGL(kmeans_scatter_kernel, dim3(w.ntiles), dim3(64), 0, st, assign, n, K, key_bits, w.hist, w.starts, w.sorted);
    // the levels: the largest cluster a call of n points can hold shrinks 64-fold per level, to one row at the last
    int levels = 0;
    for (int64_t most = n; levels == 0 || most > 1; most = (most + kKmChunk - 1) / kKmChunk) ++levels;
    int64_t bound = n;                                     // rows a level can put out, at the most (host-known: the grid)
    for (int l = 0; l < levels; ++l) {
        const int64_t out_bound = bound / kKmChunk + K < bound ? bound / kKmChunk + K : bound;
        const int nb = blocks_for(out_bound, gpb);
        const int32_t *st_in = w.starts + (size_t)l * (K + 1), *st_out = st_in + (K + 1);
        const float *src = l ? w.sums[(l - 1) & 1] : nullptr;
        float *dst = w.sums[l & 1];
        if (l == 0) {
#define CALL(LPR, NV) hipLaunchKernelGGL((kmeans_segsum_kernel<LPR, NV, true>), dim3(nb), dim3(kBlock), 0, st, W, d4, ids, w.sorted, src, st_in, st_out, K, dst)
            GLOVE_DISPATCH_ROW_SHAPE(shape, CALL);
#undef CALL
        } else {
#define CALL(LPR, NV) hipLaunchKernelGGL((kmeans_segsum_kernel<LPR, NV, false>), dim3(nb), dim3(kBlock), 0, st, W, d4, ids, w.sorted, src, st_in, st_out, K, dst)
            GLOVE_DISPATCH_ROW_SHAPE(shape, CALL);
#undef CALL
        }
        bound = out_bound;
    }
    const int nbk = blocks_for(K, gpb);
    const float *last = w.sums[(levels - 1) & 1];
    const int32_t *st_last = w.starts + (size_t)levels * (K + 1);
#define CALL(LPR, NV) hipLaunchKernelGGL((kmeans_finish_kernel<LPR, NV>), dim3(nbk), dim3(kBlock), 0, st, last, st_last, counts_out, C_in, d4, K, C_out)
    GLOVE_DISPATCH_ROW_SHAPE(shape, CALL);
#undef CALL
    return (int)hipGetLastError();
}

}  // extern "C"

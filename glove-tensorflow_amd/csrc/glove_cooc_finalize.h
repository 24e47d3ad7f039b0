// What the two finalisations of libglove_prep_hip.so share: glove_cooc_finalize (glove_cooc_stream.hip) and
// glove_cooc_finalize_weighted (glove_cooc_options.hip).  Inline functions only: every kernel stays in the one object
// that defines it.
#pragma once
#include "glove_merge_path.h"

namespace glove {

constexpr int kWindowHarmonic = 0, kWindowUniform = 1, kWindowDynamic = 2;      // GLOVE_WINDOW_* of glove_cooc_options_hip.h

// flag of entry i: 1 where a new (a, b) starts whose count reaches min_count (at most `context` keys share one (a, b))
__device__ inline int64_t finalize_head_flag(const uint64_t *__restrict__ keys, const int64_t *__restrict__ counts, int64_t m,
                                             int64_t i, int32_t context, int64_t min_count)
{
    const uint64_t ab = keys[i] / context;
    if (i != 0 && keys[i - 1] / context == ab) return 0;
    int64_t cnt = 0;
    for (int64_t j = i; j < m && j < i + context && keys[j] / context == ab; ++j) cnt += counts[j];
    return cnt >= min_count ? 1 : 0;
}

// count and value of the (a, b) that starts at entry i.  HARMONIC: sum_k (double)n_k / (double)k, k ascending from 0.0 (the
// expression and order of cooc_aggregate in glove_cooc.hip); UNIFORM and DYNAMIC sum integers and convert once.
template <int WEIGHTING>
__device__ inline void finalize_pair(const uint64_t *__restrict__ keys, const int64_t *__restrict__ counts, int64_t m, int64_t i,
                                     int32_t context, int64_t &cnt, double &val)
{
    const uint64_t ab = keys[i] / context;
    cnt = 0;
    val = 0.0;
    int64_t weighted = 0;
    for (int64_t j = i; j < m && j < i + context; ++j) {
        const uint64_t key = keys[j];
        if (key / context != ab) break;
        const int k = (int)(key % context) + 1;
        cnt += counts[j];
        if (WEIGHTING == kWindowHarmonic) val += (double)counts[j] / (double)k;
        if (WEIGHTING == kWindowDynamic) weighted += counts[j] * (int64_t)(context - k + 1);
    }
    if (WEIGHTING == kWindowUniform) val = (double)cnt;
    if (WEIGHTING == kWindowDynamic) val = (double)weighted / (double)context;
}

struct FinalizeWs {
    int64_t *flag, *incl;
    void *prim;
    size_t prim_bytes, bytes;
};

inline FinalizeWs carve_finalize_ws(void *ws, int64_t cap_keys)
{
    FinalizeWs w;
    size_t off = 0;
    char *base = (char *)ws;
    auto take = [&](size_t bytes) { void *q = base + off; off += align_up(bytes, 256); return q; };
    const size_t n = (size_t)(cap_keys > 0 ? cap_keys : 1);
    w.flag = (int64_t *)take(n * 8);
    w.incl = (int64_t *)take(n * 8);
    w.prim_bytes = (size_t)(1u << 20) + n / 16;
    w.prim = take(w.prim_bytes);
    w.bytes = off;
    return w;
}

inline bool bad_key_shape(int32_t V, int32_t context)
{
    if (V <= 0 || context <= 0 || context > 255) return true;
    return (double)V * (double)V * (double)context >= 9.0e18;      // key must fit 63 bits
}

// what both finalisations refuse before any launch
inline bool finalize_bad_args(const uint64_t *keys, const int64_t *counts, const int64_t *n, int64_t cap_keys, int32_t V,
                              int32_t context, const int32_t *out_row, const int32_t *out_col, const int64_t *out_count,
                              const double *out_value, const int64_t *out_nnz, int64_t cap_out, const void *ws)
{
    if (cap_keys < 0 || cap_keys > kMaxStateCap || bad_key_shape(V, context) || cap_out < 0 || !n || !out_nnz || !ws) return true;
    return (cap_keys > 0 && (!keys || !counts)) || (cap_out > 0 && (!out_row || !out_col || !out_count || !out_value));
}

}  // namespace glove

// Reading and writing word-vector text files on gfx950 (include/glove_vectors_hip.h, libglove_prep_hip.so).
//
// `word v1 ... vd` per line is what every other tool exchanges vectors in; a 400 k x 300 table is 1.2e8 decimal numbers.
//   vec_lines_count     one workgroup per tile of 4096 bytes, 16 B per lane: what the tile does to the line state;
//   rocPRIM scan        of the tile summaries (composition of state functions: associative, not commutative);
//   vec_lines_emit      the same summaries again; record starts numbered, the fields so far noted at every record's end;
//   vec_lines_fields    fields of a record = fields so far at its end - at the end of the record before it;
//   vec_parse           one wave per record: 64 bytes per trip, separators balloted, the lane at a field start parses it;
//   vec_format_lengths  one wave per row: the length of its text;  rocPRIM scan;  vec_format_write  writes it.
// Decimal -> float32 is one IEEE double operation on exact operands (Clinger's fast path; this unit is built without
// fast-math), float32 -> decimal is integer arithmetic below 2^64.  tests/vectors_ref.py restates both.
#include "glove_common.h"
#include "glove_merge_path.h"
#include "../../include/glove_vectors_hip.h"

#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>

namespace glove {

constexpr int kVecTile = GLOVE_VECTORS_TILE_BYTES;      // bytes per workgroup
constexpr int kVecLaneBytes = kVecTile / kBlock;        // ... per lane
static_assert(kVecLaneBytes == 16 && kVecLaneBytes * kBlock == kVecTile, "a lane reads one 16-B word");
constexpr int kWaves = kBlock / 64;
constexpr int64_t kMaxVecBytes = 2147483647;

__device__ inline bool vec_separator(uint32_t c) { return c == 0x20 || c == 0x0A || c == 0x0D; }

// ---- records ---------------------------------------------------------------------------------------------------------
// What a stretch of bytes does to the line state (0: no field since the last 0A, 1: the line has a field), for both states
// it can be entered in: rec0 / rec1 = records that start in it, bit 0 / bit 1 of out = the state it is left in; and the
// fields that start in it, which do not depend on the state.
struct LineFn { uint32_t rec0, rec1, fields, out; };

__host__ __device__ inline LineFn line_identity() { return LineFn{0u, 0u, 0u, 2u}; }

struct LineCompose {      // a, then b
    __host__ __device__ inline LineFn operator()(const LineFn &a, const LineFn &b) const
    {
        const uint32_t a0 = a.out & 1u, a1 = (a.out >> 1) & 1u;
        LineFn c;
        c.rec0 = a.rec0 + (a0 ? b.rec1 : b.rec0);
        c.rec1 = a.rec1 + (a1 ? b.rec1 : b.rec0);
        c.fields = a.fields + b.fields;
        c.out = ((b.out >> a0) & 1u) | (((b.out >> a1) & 1u) << 1);
        return c;
    }
};

// This lane's 16 bytes of the tile as masks: bit i set where byte base + i is no separator / is 0A / starts a field.
// Returns how many of the 16 lie inside the block.
__device__ inline int lane_masks(const uint8_t *__restrict__ bytes, int64_t n, int64_t base, uint32_t &nonsep, uint32_t &lf,
                                 uint32_t &fstart)
{
    nonsep = lf = fstart = 0u;
    if (base >= n) return 0;
    const int own = base + kVecLaneBytes <= n ? kVecLaneBytes : (int)(n - base);
    uint32_t word[4] = {0u, 0u, 0u, 0u};
    if (((uintptr_t)bytes & 15) == 0 && own == kVecLaneBytes) {
        const uint4 v = *(const uint4 *)(bytes + base);
        word[0] = v.x; word[1] = v.y; word[2] = v.z; word[3] = v.w;
    } else {                                 // the block's tail, or a block that does not start on a 16-B boundary
        for (int i = 0; i < own; ++i) word[i >> 2] |= (uint32_t)bytes[base + i] << (8 * (i & 3));
    }
#pragma unroll
    for (int i = 0; i < kVecLaneBytes; ++i) {
        const uint32_t c = (word[i >> 2] >> (8 * (i & 3))) & 255u;
        if (i < own) {
            if (c == 0x0A) lf |= 1u << i;
            if (!vec_separator(c)) nonsep |= 1u << i;
        }
    }
    const bool prev_field = base > 0 && !vec_separator(bytes[base - 1]);
    fstart = nonsep & ~((nonsep << 1) | (prev_field ? 1u : 0u));
    return own;
}

__device__ inline LineFn lane_fn(uint32_t nonsep, uint32_t lf, uint32_t fstart)
{
    uint32_t s0 = 0u, s1 = 1u, r0 = 0u, r1 = 0u;
#pragma unroll
    for (int i = 0; i < kVecLaneBytes; ++i) {
        if ((lf >> i) & 1u) {
            s0 = s1 = 0u;
        } else if ((nonsep >> i) & 1u) {      // a field byte in state 0 starts a record
            r0 += s0 ^ 1u;
            r1 += s1 ^ 1u;
            s0 = s1 = 1u;
        }
    }
    return LineFn{r0, r1, (uint32_t)__popc(fstart), s0 | (s1 << 1)};
}

__device__ inline LineFn shfl_up_fn(const LineFn &v, int dlt)
{
    return LineFn{(uint32_t)__shfl_up((int)v.rec0, dlt, 64), (uint32_t)__shfl_up((int)v.rec1, dlt, 64),
                  (uint32_t)__shfl_up((int)v.fields, dlt, 64), (uint32_t)__shfl_up((int)v.out, dlt, 64)};
}

// before = the composition of the lanes in front of this one, total = of the whole workgroup.  Holds a __syncthreads.
__device__ inline void block_scan_fn(const LineFn &mine, LineFn *s_wave, LineFn &before, LineFn &total)
{
    const LineCompose then;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    LineFn incl = mine;
#pragma unroll
    for (int dlt = 1; dlt < 64; dlt <<= 1) {
        const LineFn up = shfl_up_fn(incl, dlt);
        if (lane >= dlt) incl = then(up, incl);
    }
    LineFn excl = shfl_up_fn(incl, 1);
    if (lane == 0) excl = line_identity();
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    before = total = line_identity();
#pragma unroll
    for (int wv = 0; wv < kWaves; ++wv) {
        if (wv < wave) before = then(before, s_wave[wv]);
        total = then(total, s_wave[wv]);
    }
    before = then(before, excl);
}

__global__ __launch_bounds__(kBlock) void vec_lines_count(const uint8_t *__restrict__ bytes, int64_t n, LineFn *__restrict__ summary)
{
    __shared__ LineFn s_wave[kWaves];
    uint32_t nonsep, lf, fstart;
    lane_masks(bytes, n, (int64_t)blockIdx.x * kVecTile + (int64_t)threadIdx.x * kVecLaneBytes, nonsep, lf, fstart);
    LineFn before, total;
    block_scan_fn(lane_fn(nonsep, lf, fstart), s_wave, before, total);
    if (threadIdx.x == 0) summary[blockIdx.x] = total;
}

// prefix[tile] = the composition of the tiles in front of it; the block is entered in state 0.  cum[r] = the fields that
// started up to the end of record r: written where the record ends, at a 0A or at the block's end, wherever it started.
__global__ __launch_bounds__(kBlock) void vec_lines_emit(const uint8_t *__restrict__ bytes, int64_t n,
                                                         const LineFn *__restrict__ prefix, int32_t *__restrict__ line_start,
                                                         int32_t *__restrict__ cum, int64_t *__restrict__ n_lines, int64_t cap)
{
    __shared__ LineFn s_wave[kWaves];
    const int64_t base = (int64_t)blockIdx.x * kVecTile + (int64_t)threadIdx.x * kVecLaneBytes;
    uint32_t nonsep, lf, fstart;
    const int own = lane_masks(bytes, n, base, nonsep, lf, fstart);
    LineFn before, total;
    block_scan_fn(lane_fn(nonsep, lf, fstart), s_wave, before, total);
    const LineFn pre = prefix[blockIdx.x];
    const uint32_t tile_state = pre.out & 1u;
    if (threadIdx.x == 0 && blockIdx.x == gridDim.x - 1) *n_lines = (int64_t)pre.rec0 + (tile_state ? total.rec1 : total.rec0);
    int64_t r = (int64_t)pre.rec0 + (tile_state ? before.rec1 : before.rec0);      // records that started in front of this lane
    uint32_t f = pre.fields + before.fields;                                        // fields likewise
    uint32_t state = (before.out >> tile_state) & 1u;
#pragma unroll
    for (int i = 0; i < kVecLaneBytes; ++i) {
        f += (fstart >> i) & 1u;
        if ((lf >> i) & 1u) {
            if (state && r - 1 < cap) cum[r - 1] = (int32_t)f;
            state = 0u;
        } else if (((nonsep >> i) & 1u) && !state) {
            if (r < cap) line_start[r] = (int32_t)(base + i);
            ++r;
            state = 1u;
        }
    }
    if (own > 0 && base + own == n && state && r - 1 < cap) cum[r - 1] = (int32_t)f;      // the block's end ends a record
}

__global__ void vec_lines_fields(const int32_t *__restrict__ cum, const int64_t *__restrict__ n_lines, int64_t cap,
                                 int32_t *__restrict__ line_fields)
{
    const int64_t m = clamp_count(n_lines, cap);
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < m; r += (int64_t)gridDim.x * blockDim.x)
        line_fields[r] = cum[r] - (r > 0 ? cum[r - 1] : 0);
}

struct LinesWs {
    LineFn *summary, *prefix;
    int32_t *cum;
    void *prim;
    size_t prim_bytes, bytes;
    int64_t tiles, lines;
};

static LinesWs carve_lines_ws(void *ws, int64_t n_bytes, int64_t cap)
{
    LinesWs w;
    WsCarver c{(char *)ws};
    w.tiles = (n_bytes + kVecTile - 1) / kVecTile;
    if (w.tiles < 1) w.tiles = 1;
    w.lines = cap < (n_bytes + 1) / 2 ? cap : (n_bytes + 1) / 2;
    if (w.lines < 1) w.lines = 1;
    w.summary = c.take<LineFn>((size_t)w.tiles);
    w.prefix = c.take<LineFn>((size_t)w.tiles);
    w.cum = c.take<int32_t>((size_t)w.lines);
    w.prim_bytes = (size_t)(64u << 10) + (size_t)w.tiles * 16;
    w.prim = c.take<char>(w.prim_bytes);
    w.bytes = c.off;
    return w;
}

// ---- decimal -> float32 ----------------------------------------------------------------------------------------------
__device__ const double kPow10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                      1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};

// The token that starts at byte p: its length in `len`; true and its value in `out` where the fast path holds.
__device__ inline bool parse_decimal(const uint8_t *__restrict__ b, int64_t n, int64_t p, float &out, int64_t &len)
{
    int64_t q = p;
    auto peek = [&]() -> uint32_t { return q < n ? (uint32_t)b[q] : 0x20u; };
    auto digit = [](uint32_t c) { return c >= '0' && c <= '9'; };
    uint32_t c = peek();
    bool neg = false;
    if (c == '+' || c == '-') { neg = c == '-'; ++q; c = peek(); }
    uint64_t m = 0;
    int nd = 0;                   // significant digits: those from the first nonzero one on
    int64_t fd = 0;               // digits behind the '.'
    bool any = false, dot = false, ok = true;
    for (;; ++q, c = peek()) {
        if (digit(c)) {
            any = true;
            if (m != 0 || c != '0') {
                if (nd < 15) m = m * 10 + (c - '0');
                ++nd;
            }
            if (dot) ++fd;
        } else if (c == '.' && !dot) {
            dot = true;
        } else {
            break;
        }
    }
    int64_t ex = 0;
    if (any && (c == 'e' || c == 'E')) {
        ++q; c = peek();
        bool eneg = false, edigit = false;
        if (c == '+' || c == '-') { eneg = c == '-'; ++q; c = peek(); }
        while (digit(c)) {
            edigit = true;
            if (ex < 100000) ex = ex * 10 + (c - '0');
            ++q; c = peek();
        }
        ok = edigit;
        if (eneg) ex = -ex;
    }
    ok = ok && any && vec_separator(c);       // the grammar, and nothing behind it
    while (!vec_separator(peek())) ++q;
    len = q - p;
    if (!ok || nd > 15) return false;
    double v = 0.0;
    if (m != 0) {
        const int64_t e10 = ex - fd;
        if (e10 < -22 || e10 > 22) return false;
        v = e10 >= 0 ? (double)m * kPow10[e10] : (double)m / kPow10[-e10];
    }
    out = (float)(neg ? -v : v);
    return true;
}

__global__ __launch_bounds__(kBlock) void vec_parse(const uint8_t *__restrict__ bytes, int64_t n, const int32_t *__restrict__ line_start,
                                                    const int64_t *__restrict__ n_lines, int64_t cap_lines, int d, int ld,
                                                    float *__restrict__ vec, int32_t *__restrict__ word_len,
                                                    int64_t *__restrict__ fb_index, int64_t *__restrict__ fb_span,
                                                    int64_t *__restrict__ n_fallback, int64_t cap_fb)
{
    const int lane = threadIdx.x & 63;
    const int64_t m = clamp_count(n_lines, cap_lines);
    const int64_t waves = (int64_t)gridDim.x * kWaves;
    for (int64_t r = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); r < m; r += waves) {      // (r is the same in a wave)
        float *__restrict__ row = vec + r * ld;
        const int64_t s = line_start[r];
        int fields = 0, wlen = -1;                  // field starts so far; the word's length once its end was seen
        if (s >= 0 && s < n) {
            bool prev_sep = true, done = false;
            for (int64_t p0 = s; !done; p0 += 64) {
                const int64_t p = p0 + lane;
                const uint32_t c = p < n ? (uint32_t)bytes[p] : 0x0Au;        // the block's end ends the record
                const unsigned long long sepm = __ballot(vec_separator(c)), lfm = __ballot(c == 0x0A);
                const unsigned long long live = lfm ? (lfm & (~lfm + 1ull)) - 1ull : ~0ull;      // the bytes in front of the first 0A
                const unsigned long long startm = ~sepm & ((sepm << 1) | (prev_sep ? 1ull : 0ull)) & live;
                if (wlen < 0 && sepm) wlen = (int)(p0 - s) + __ffsll((long long)sepm) - 1;
                if ((startm >> lane) & 1ull) {
                    const int j = fields + __popcll(startm & ((1ull << lane) - 1ull));      // this field's number
                    if (j >= 1 && j <= d) {
                        float v;
                        int64_t len;
                        if (parse_decimal(bytes, n, p, v, len)) {
                            row[j - 1] = v;
                        } else {
                            const int64_t k = (int64_t)atomicAdd((unsigned long long *)n_fallback, 1ull);
                            if (k < cap_fb) {
                                fb_index[k] = r * ld + (j - 1);
                                fb_span[k] = (p << 16) | (len < GLOVE_VECTORS_MAX_SPAN ? len : GLOVE_VECTORS_MAX_SPAN);
                            }
                        }
                    }
                }
                fields += __popcll(startm);
                prev_sep = (sepm >> 63) & 1ull;
                done = lfm != 0ull;
            }
        }
        const int filled = fields - 1 < 0 ? 0 : (fields - 1 < d ? fields - 1 : d);
        for (int col = filled + lane; col < ld; col += 64) row[col] = 0.f;      // missing fields and the padding columns
        if (lane == 0) word_len[r] = wlen < 0 ? 0 : wlen;
    }
}

// ---- float32 -> fixed decimal ----------------------------------------------------------------------------------------
__device__ const uint64_t kPow10u[10] = {1ull, 10ull, 100ull, 1000ull, 10000ull, 100000ull, 1000000ull, 10000000ull,
                                         100000000ull, 1000000000ull};

// q = |x| 10^p rounded to the nearest integer, ties to even; false for a NaN, an infinity or |x| >= 2^31
__device__ inline bool fixed_q(uint32_t bits, uint64_t pow10p, uint64_t &q)
{
    const uint32_t e = (bits >> 23) & 255u, frac = bits & 0x7FFFFFu;
    if (e == 255u) return false;
    const uint64_t m = e ? (uint64_t)(frac | 0x800000u) : (uint64_t)frac;
    const int ex = e ? (int)e - 150 : -149;
    if (ex >= 8) return false;
    const uint64_t nn = m * pow10p;           // < 2^24 10^9 < 2^54
    if (ex >= 0) { q = nn << ex; return true; }
    const int s = -ex;
    if (s >= 64) { q = 0; return true; }
    q = nn >> s;
    const uint64_t rem = nn & ((1ull << s) - 1ull), half = 1ull << (s - 1);
    if (rem > half || (rem == half && (q & 1ull))) ++q;
    return true;
}

__device__ inline int decimal_digits(uint64_t v)
{
    int k = 1;
    while (v >= 10) { v /= 10; ++k; }
    return k;
}

// bytes of " " + the text of the value
__device__ inline int value_length(uint32_t bits, uint64_t q, int p, uint64_t pow10p)
{
    return 1 + (int)(bits >> 31) + decimal_digits(q / pow10p) + (p > 0 ? 1 + p : 0);
}

__global__ __launch_bounds__(kBlock) void vec_format_lengths(const float *__restrict__ W, int64_t n_rows, int d, int ld, int p,
                                                             const int64_t *__restrict__ word_off, int64_t *__restrict__ row_len,
                                                             uint8_t *__restrict__ host_row, int64_t *__restrict__ n_host_rows)
{
    const int lane = threadIdx.x & 63;
    const uint64_t pow10p = kPow10u[p];
    if (blockIdx.x == 0 && threadIdx.x == 0) row_len[n_rows] = 0;          // the scan's last slot: row_off[n_rows] = the size
    const int64_t waves = (int64_t)gridDim.x * kWaves;
    for (int64_t r = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); r < n_rows; r += waves) {
        const uint32_t *__restrict__ row = (const uint32_t *)(W + r * ld);
        bool host = false;
        int len = 0;
        for (int col = lane; col < d; col += 64) {
            const uint32_t bits = row[col];
            uint64_t q;
            if (fixed_q(bits, pow10p, q)) len += value_length(bits, q, p, pow10p);
            else host = true;
        }
        host = __ballot(host) != 0ull;
        len = wave_sum_int(len);
        if (lane == 0) {
            row_len[r] = host ? 0 : (word_off[r + 1] - word_off[r]) + len + 1;
            host_row[r] = host ? 1 : 0;
            if (host) atomicAdd((unsigned long long *)n_host_rows, 1ull);
        }
    }
}

__global__ __launch_bounds__(kBlock) void vec_format_write(const float *__restrict__ W, int64_t n_rows, int d, int ld, int p,
                                                           const uint8_t *__restrict__ word_bytes, const int64_t *__restrict__ word_off,
                                                           const int64_t *__restrict__ row_off, const uint8_t *__restrict__ host_row,
                                                           uint8_t *__restrict__ out, int64_t cap_out)
{
    const int lane = threadIdx.x & 63;
    const uint64_t pow10p = kPow10u[p];
    auto put = [&](int64_t o, uint32_t ch) { if (o < cap_out) out[o] = (uint8_t)ch; };
    const int64_t waves = (int64_t)gridDim.x * kWaves;
    for (int64_t r = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); r < n_rows; r += waves) {
        if (host_row[r]) continue;
        const uint32_t *__restrict__ row = (const uint32_t *)(W + r * ld);
        int64_t pos = row_off[r];
        const int64_t w0 = word_off[r], wl = word_off[r + 1] - w0;
        for (int64_t i = lane; i < wl; i += 64) put(pos + i, word_bytes[w0 + i]);
        pos += wl;
        for (int c0 = 0; c0 < d; c0 += 64) {
            const int col = c0 + lane;
            uint32_t bits = 0u;
            uint64_t q = 0;
            int mine = 0;
            if (col < d) {
                bits = row[col];
                fixed_q(bits, pow10p, q);
                mine = value_length(bits, q, p, pow10p);
            }
            int incl = mine;
#pragma unroll
            for (int dlt = 1; dlt < 64; dlt <<= 1) {
                const int up = __shfl_up(incl, dlt, 64);
                if (lane >= dlt) incl += up;
            }
            if (col < d) {
                int64_t o = pos + incl - mine;
                put(o++, ' ');
                if (bits >> 31) put(o++, '-');
                uint64_t ip = q / pow10p, fp = q % pow10p;
                const int nd = decimal_digits(ip);
                for (int k = nd - 1; k >= 0; --k) { put(o + k, '0' + (uint32_t)(ip % 10)); ip /= 10; }
                o += nd;
                if (p > 0) {
                    put(o++, '.');
                    for (int k = p - 1; k >= 0; --k) { put(o + k, '0' + (uint32_t)(fp % 10)); fp /= 10; }
                }
            }
            pos += __shfl(incl, 63, 64);
        }
        if (lane == 0) put(pos, 0x0A);
    }
}

struct FormatWs {
    int64_t *row_len;
    void *prim;
    size_t prim_bytes, bytes;
};

static FormatWs carve_format_ws(void *ws, int64_t n_rows)
{
    FormatWs w;
    WsCarver c{(char *)ws};
    w.row_len = c.take<int64_t>((size_t)n_rows + 1);
    w.prim_bytes = (size_t)(64u << 10) + ((size_t)n_rows + 1) * 8;
    w.prim = c.take<char>(w.prim_bytes);
    w.bytes = c.off;
    return w;
}

// one wave per item, kWaves to a workgroup
static int wave_blocks(int64_t items) { return blocks_for(items, kWaves); }

}  // namespace glove

using namespace glove;

extern "C" {

int glove_vectors_abi_version(void) { return GLOVE_VECTORS_ABI_VERSION; }

size_t glove_vectors_lines_workspace_bytes(int64_t n_bytes, int64_t cap)
{
    if (n_bytes < 0 || n_bytes > kMaxVecBytes || cap < 0) return 0;
    return carve_lines_ws(nullptr, n_bytes, cap).bytes;
}

int glove_vectors_lines_u8(const uint8_t *bytes, int64_t n_bytes, int32_t *line_start, int32_t *line_fields, int64_t *n_lines,
                           int64_t cap, void *ws, size_t ws_bytes, void *stream)
{
    if (n_bytes < 0 || n_bytes > kMaxVecBytes || cap < 0 || !n_lines || !ws) return GLOVE_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    if (n_bytes == 0) {
        HIP_TRY(zero_words(n_lines, 2, st));
        return 0;
    }
    if (!bytes || (cap > 0 && (!line_start || !line_fields))) return GLOVE_E_BADARG;
    const LinesWs w = carve_lines_ws(ws, n_bytes, cap);
    if (w.bytes > ws_bytes) return GLOVE_E_WORKSPACE;
    size_t need = 0;
    HIP_TRY(rocprim::exclusive_scan(nullptr, need, w.summary, w.prefix, line_identity(), (size_t)w.tiles, LineCompose(), st));
    if (need > w.prim_bytes) return GLOVE_E_WORKSPACE;
    const dim3 grid((unsigned int)w.tiles);
    hipLaunchKernelGGL(vec_lines_count, grid, dim3(kBlock), 0, st, bytes, n_bytes, w.summary);
    HIP_TRY(rocprim::exclusive_scan(w.prim, need, w.summary, w.prefix, line_identity(), (size_t)w.tiles, LineCompose(), st));
    hipLaunchKernelGGL(vec_lines_emit, grid, dim3(kBlock), 0, st, bytes, n_bytes, w.prefix, line_start, w.cum, n_lines, cap);
    // n_lines lives on the device: the last pass is sized by the capacity (and by the most records the bytes can hold)
    if (cap > 0)
        hipLaunchKernelGGL(vec_lines_fields, dim3(blocks_for(w.lines, kBlock)), dim3(kBlock), 0, st, w.cum, n_lines, w.lines,
                           line_fields);
    return (int)hipGetLastError();
}

int glove_vectors_parse_f32(const uint8_t *bytes, int64_t n_bytes, const int32_t *line_start, const int64_t *n_lines,
                            int64_t cap_lines, int32_t d, int32_t ld, float *vec, int32_t *word_len, int64_t *fb_index,
                            int64_t *fb_span, int64_t *n_fallback, int64_t cap_fb, void *stream)
{
    if (n_bytes < 0 || n_bytes > kMaxVecBytes || cap_lines < 0 || cap_lines > kMaxVecBytes || cap_fb < 0 || d < 1 ||
        d > GLOVE_VECTORS_MAX_D || ld < d || ld % 4 != 0 || !n_lines || !n_fallback)
        return GLOVE_E_BADARG;
    if ((cap_lines > 0 && (!line_start || !vec || !word_len || (n_bytes > 0 && !bytes))) || (cap_fb > 0 && (!fb_index || !fb_span)))
        return GLOVE_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(zero_words(n_fallback, 2, st));
    if (cap_lines == 0 || n_bytes == 0) return 0;
    const int64_t most = cap_lines < (n_bytes + 1) / 2 ? cap_lines : (n_bytes + 1) / 2;
    hipLaunchKernelGGL(vec_parse, dim3(wave_blocks(most)), dim3(kBlock), 0, st, bytes, n_bytes, line_start, n_lines, cap_lines,
                       (int)d, (int)ld, vec, word_len, fb_index, fb_span, n_fallback, cap_fb);
    return (int)hipGetLastError();
}

size_t glove_vectors_format_workspace_bytes(int64_t n_rows, int32_t d)
{
    if (n_rows < 0 || n_rows > kMaxVecBytes || d < 1 || d > GLOVE_VECTORS_MAX_D) return 0;
    return carve_format_ws(nullptr, n_rows).bytes;
}

int glove_vectors_format_f32(const float *W, int64_t n_rows, int32_t d, int32_t ld, int32_t precision,
                             const uint8_t *word_bytes, const int64_t *word_off, uint8_t *out, int64_t *row_off,
                             uint8_t *host_row, int64_t *n_host_rows, int64_t cap_out, void *ws, size_t ws_bytes, void *stream)
{
    if (n_rows < 0 || n_rows > kMaxVecBytes || d < 1 || d > GLOVE_VECTORS_MAX_D || ld < d || precision < 0 || precision > 9 ||
        cap_out < 0 || !word_off || !row_off || !n_host_rows || !ws)
        return GLOVE_E_BADARG;
    if ((n_rows > 0 && (!W || !host_row)) || (cap_out > 0 && !out)) return GLOVE_E_BADARG;
    const FormatWs w = carve_format_ws(ws, n_rows);
    if (w.bytes > ws_bytes) return GLOVE_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const size_t slots = (size_t)n_rows + 1;
    size_t need = 0;
    HIP_TRY(rocprim::exclusive_scan(nullptr, need, w.row_len, row_off, (int64_t)0, slots, rocprim::plus<int64_t>(), st));
    if (need > w.prim_bytes) return GLOVE_E_WORKSPACE;
    HIP_TRY(zero_words(n_host_rows, 2, st));
    const dim3 grid(wave_blocks(n_rows));
    hipLaunchKernelGGL(vec_format_lengths, grid, dim3(kBlock), 0, st, W, n_rows, (int)d, (int)ld, (int)precision, word_off,
                       w.row_len, host_row, n_host_rows);
    HIP_TRY(rocprim::exclusive_scan(w.prim, need, w.row_len, row_off, (int64_t)0, slots, rocprim::plus<int64_t>(), st));
    if (n_rows > 0 && cap_out > 0)
        hipLaunchKernelGGL(vec_format_write, grid, dim3(kBlock), 0, st, W, n_rows, (int)d, (int)ld, (int)precision, word_bytes,
                           word_off, row_off, host_row, out, cap_out);
    return (int)hipGetLastError();
}

}  // extern "C"

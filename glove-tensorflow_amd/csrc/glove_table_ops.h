// What the objects of libglove_prep_hip.so share beyond inline helpers (glove_merge_path.h):
//   - the two operations on a sorted (key, payload) table that more than one entry point runs, the merge-path merge and the
//     finalisation.  Their kernels are compiled once, in glove_table_ops.hip; the entry points of glove_cooc_stream.hip,
//     glove_text.hip and glove_cooc_options.hip pack their arguments and call the host drivers declared here (host calls
//     across objects: no relocatable device code);
//   - the workspace of a count pass / scan / write pass over tiles, and rocPRIM's scan of the tile counts (the token filter's, the
//     phrase selection's; the phrase join carves the same pieces for its running maximum over tiles).
#pragma once
#include "glove_merge_path.h"

#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>

namespace glove {

// ---- tile counts -----------------------------------------------------------------------------------------------------
// count[tiles] | offset[tiles] | 64 KiB + 8 tiles of scan scratch: a first pass leaves every tile's number of outputs in
// count, the scan makes offset of them, a second pass writes tile t's outputs at offset[t]
struct TileCounts {
    int64_t *count, *offset;
    void *prim;
    size_t prim_bytes;
    int64_t tiles;
};

// the tiles of per_tile items that cover `items` (an empty input still has one)
inline int64_t tiles_of(int64_t items, int64_t per_tile)
{
    const int64_t tiles = (items + per_tile - 1) / per_tile;
    return tiles < 1 ? 1 : tiles;
}

inline TileCounts carve_tile_counts(WsCarver &c, int64_t tiles)
{
    TileCounts t;
    t.tiles = tiles;
    t.count = c.take<int64_t>((size_t)t.tiles);
    t.offset = c.take<int64_t>((size_t)t.tiles);
    t.prim_bytes = (size_t)(64u << 10) + (size_t)t.tiles * 8;
    t.prim = c.take<char>(t.prim_bytes);
    return t;
}

// the bytes of a workspace that holds nothing else
inline size_t tile_counts_bytes(int64_t tiles)
{
    WsCarver c{nullptr};
    carve_tile_counts(c, tiles);
    return c.off;
}

// offset = the exclusive scan of count, with rocPRIM's own convention: prim == nullptr only sets `need`, nothing is launched
inline hipError_t tile_scan(const TileCounts &t, void *prim, size_t &need, hipStream_t st)
{
    return rocprim::exclusive_scan(prim, need, t.count, t.offset, (int64_t)0, (size_t)t.tiles, rocprim::plus<int64_t>(), st);
}

// need = the scratch the scan wants; GLOVE_E_WORKSPACE where the carve holds less.  Then: HIP_TRY(tile_scan(t, t.prim, need, st)).
inline int tile_scan_query(const TileCounts &t, size_t &need, hipStream_t st)
{
    need = 0;
    HIP_TRY(tile_scan(t, nullptr, need, st));
    return need > t.prim_bytes ? GLOVE_E_WORKSPACE : 0;
}

// the drivers are the library's own: reached from its other objects, not from outside it
#define GLOVE_PREP_LOCAL __attribute__((visibility("hidden")))

// ---- merge -----------------------------------------------------------------------------------------------------------
// A sorted, duplicate-free table: cap slots, *n of them used (a device-side count), npay payload words beside every key
constexpr int kMaxPayloads = 2;
struct MergeIn {
    const uint64_t *keys;
    const int64_t *pay[kMaxPayloads];
    const int64_t *n;
    int64_t cap;
};
struct MergeOut {
    uint64_t *keys;
    int64_t *pay[kMaxPayloads];
    int64_t *n;
    int64_t cap;
};

// 0 where a capacity is refused
GLOVE_PREP_LOCAL size_t merge_workspace_bytes(int64_t cap_a, int64_t cap_b);
// out = a merged with b.  A key both hold appears once: its payload 0 is the sum of the two, its payload 1 the smaller one.
// Partition, count pass, scan, write pass: four launches and the scan's on st, nothing read back.
GLOVE_PREP_LOCAL int merge_tables(const MergeIn &a, const MergeIn &b, const MergeOut &out, int npay, void *ws, size_t ws_bytes,
                                  hipStream_t st);

// ---- finalize --------------------------------------------------------------------------------------------------------
constexpr int kWindowHarmonic = 0, kWindowUniform = 1, kWindowDynamic = 2;      // GLOVE_WINDOW_* of glove_cooc_options_hip.h

GLOVE_PREP_LOCAL size_t finalize_workspace_bytes(int64_t cap_keys);
// the (row, col, count, value) table of a state of (key, count): mark, scan, aggregate<weighting>; weighting is a kWindow*
GLOVE_PREP_LOCAL int finalize_table(const uint64_t *keys, const int64_t *counts, const int64_t *n, int64_t cap_keys, int32_t V,
                                    int32_t context, int64_t min_count, int weighting, int32_t *out_row, int32_t *out_col,
                                    int64_t *out_count, double *out_value, int64_t *out_nnz, int64_t cap_out, void *ws,
                                    size_t ws_bytes, hipStream_t st);

}  // namespace glove

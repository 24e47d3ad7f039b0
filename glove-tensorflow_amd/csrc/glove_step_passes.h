// The gather passes of the step library — sidepass_kernel, what its launches pass and the ladder that picks a build — with the
// row loads and stores and the optimizer arithmetic they share with the rest of glove_step.hip.  sidepass_kernel's builds are
// spread over four objects by shape (launch_passes, glove_step.hip), each build in exactly one of them.
#pragma once
#include "glove_common.h"
#include <type_traits>

namespace glove {

template <int LPR, int NV>
__device__ inline void load_row(f4 (&dst)[NV], const float *table, int32_t id, int d4, int lg)
{
    // branch-free: lanes past the row end re-read its last float4 and are zeroed by a select
    // (a predicated load makes hipcc branch around every row load and serialise its waits)
    const f4 *p = reinterpret_cast<const f4 *>(table) + (size_t)id * d4;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int i4 = lg + k * LPR;
        const f4 v = p[i4 < d4 ? i4 : d4 - 1];
        dst[k] = (i4 < d4) ? v : f4{0.f, 0.f, 0.f, 0.f};
    }
}

// Gather-pass row load: 32-bit byte offsets off a uniform base (tables < 4 GiB, checked on the
// host) so the compiler can use the SGPR-base + VGPR-offset load form instead of 64-bit pointer
// arithmetic per row; FULL (d4 == LPR*NV) drops the row-end predicate altogether, otherwise only the
// last float4 slot of a lane can lie past the row end.
template <int LPR, int NV, bool FULL>
__device__ inline void load_row_fast(f4 (&dst)[NV], const float *table, int32_t id, int d4, int lg)
{
    const char *base = reinterpret_cast<const char *>(table);
    const uint32_t row_bytes = FULL ? (uint32_t)(LPR * NV * 16) : (uint32_t)d4 * 16u;
    const uint32_t off = (uint32_t)id * row_bytes + (uint32_t)lg * 16u;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        if (FULL || k < NV - 1) {
            dst[k] = *reinterpret_cast<const f4 *>(base + (off + (uint32_t)(k * LPR * 16)));
        } else {
            const int i4 = lg + k * LPR;
            const uint32_t o = (uint32_t)id * row_bytes + (uint32_t)(i4 < d4 ? i4 : d4 - 1) * 16u;
            const f4 v = *reinterpret_cast<const f4 *>(base + o);
            dst[k] = (i4 < d4) ? v : f4{0.f, 0.f, 0.f, 0.f};
        }
    }
}

template <int LPR, int NV>
__device__ inline void store_row(float *table, size_t row_index, int d4, int lg, const f4 (&src)[NV])
{
    f4 *p = reinterpret_cast<f4 *>(table) + row_index * d4;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int i4 = lg + k * LPR;
        if (i4 < d4) p[i4] = src[k];
    }
}

// ---- cache policy of the run-merged (fused) passes ----------------------------------------------------------------------
// A fused pass is bound by the bytes its partner gathers miss the XCD's 4 MB L2 with: the L2 is worth what it
// holds of the Zipf head of the partner table, and everything else that streams through it — the own rows and accumulator rows,
// read once, and the finished rows and accumulators, written once and read by nobody in this launch — pushes those rows out.
// So the streams are marked: own rows and accumulators are loaded non-temporal (`nt`: served by the L2, first in line to be
// replaced), finished rows are stored write-through (`sc1`: the line does not stay in the L2; MI355X_MICROARCH.md, stores of
// each flavour).  Same bits; one process, same resident plans, twin form, us per step (tools/ab_kernels.py,
// profiles/r05_exp_cache_policy_fused_passes.txt):
//                                   plain    sc1 stores   nt loads   both
//   V = 400 k, d = 300, B = 1 M     585.1      582.1       575.8     571.2
//   V = 2 M,   d = 128, B = 1 M     377.0      372.6       372.2     368.0
// (nt on the pair fields and chunk descriptors as well: 571.6 / 369.9 — nothing, not taken; nt on the partner gathers of cold
// ids lost in round 3: DESIGN_APPENDIX.md)
template <int LPR, int NV>
__device__ inline void load_row_nt(f4 (&dst)[NV], const float *table, int32_t id, int d4, int lg)
{
    const f4 *p = reinterpret_cast<const f4 *>(table) + (size_t)id * d4;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int i4 = lg + k * LPR;
        const f4 v = __builtin_nontemporal_load(p + (i4 < d4 ? i4 : d4 - 1));
        dst[k] = (i4 < d4) ? v : f4{0.f, 0.f, 0.f, 0.f};
    }
}

template <int LPR, int NV>
__device__ inline void store_row_wt(float *table, size_t row_index, int d4, int lg, const f4 (&src)[NV])
{
    f4 *p = reinterpret_cast<f4 *>(table) + row_index * d4;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int i4 = lg + k * LPR;
        // (a store the compiler does not count in vmcnt: its own waits can only become longer by it, never shorter)
        if (i4 < d4) asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p + i4), "v"(src[k]) : "memory");
    }
}

// ---- optimizer arithmetic (Keras-legacy forms) -------------------------
// x / (sqrt(a) + eps) uses the hardware v_sqrt_f32 / v_rcp_f32 (1 ulp each) instead of the IEEE
// expansions: ~3 ulp on the update term, far inside the 1e-5 parity tolerance, and a third of the
// instructions and registers of the apply kernels.
__device__ inline float inv_sqrt_eps(float a, float eps) { return __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf(a) + eps); }

__device__ inline void adagrad_elem(float &Wv, float &A, float g, float lr, float eps)
{
    A += g * g;
    Wv -= lr * g * inv_sqrt_eps(A, eps);
}

__device__ inline void adagrad_vec(f4 &Wv, f4 &A, const f4 g, float lr, float eps)
{
    A += g * g;
    const f4 inv = f4{inv_sqrt_eps(A.x, eps), inv_sqrt_eps(A.y, eps), inv_sqrt_eps(A.z, eps), inv_sqrt_eps(A.w, eps)};
    Wv -= (lr * g) * inv;
}

// Adam's update has two products feeding one sum, which the compiler may contract either way: the rounding
// sequence is spelled out so that every kernel that applies it (dense sweep, fused step) gives the same bits.
__device__ inline void adam_elem(float &Wv, float &M, float &Vv, float g, float lr_t, float b1, float b2, float eps)
{
#pragma clang fp contract(off)
    const float g1 = (1.0f - b1) * g;
    const float g2 = ((1.0f - b2) * g) * g;
    M = __builtin_fmaf(b1, M, g1);
    Vv = __builtin_fmaf(b2, Vv, g2);
    const float step = lr_t * M;
    Wv = __builtin_fmaf(-step, inv_sqrt_eps(Vv, eps), Wv);
}

__device__ inline void adam_vec(f4 &Wv, f4 &M, f4 &Vv, const f4 g, float lr_t, float b1, float b2, float eps)
{
    float w[4] = {Wv.x, Wv.y, Wv.z, Wv.w}, m[4] = {M.x, M.y, M.z, M.w}, v[4] = {Vv.x, Vv.y, Vv.z, Vv.w};
    const float gg[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) adam_elem(w[i], m[i], v[i], gg[i], lr_t, b1, b2, eps);
    Wv = f4{w[0], w[1], w[2], w[3]};
    M = f4{m[0], m[1], m[2], m[3]};
    Vv = f4{v[0], v[1], v[2], v[3]};
}

__device__ inline float adam_lr_t(float lr, double ln_beta1, double ln_beta2, int64_t step)
{
    // 1 - beta^t = -expm1(t ln beta), logs from the host in fp64 (two fp64 pow per thread were a third of the dense sweep)
    const double t = (double)step;
    return lr * sqrtf(-expm1f((float)(t * ln_beta2))) / -expm1f((float)(t * ln_beta1));
}

// ------------------------------------------------------------------------------------------
// Gather passes: one GROUP of LPR lanes per chunk, 64/LPR chunks per wave, BOTH sides in one launch.
//
// The two sides are symmetric and independent.  A row-side chunk (row u, pairs i) gathers the
// partner rows C[col_i]; a col-side chunk (col v, pairs i) gathers R[row_i].  Either side forms
// p_i = own . partner + own_bias + partner_bias + g and e_i = 2 w_i (p_i - y_i) / B by itself (the plan
// carries w, y in both orders), so the col side needs nothing the row side produces: the first
// blocks of the grid take the row chunks, the rest the col chunks, and a step is TWO dependent kernels
// (passes -> apply) instead of three.  The second dot product per pair is cheap next to a kernel
// boundary in the latency-bound regime (B = 131072, d = 64: 9.7 + 7.5 us as two kernels, ~10 us fused).
//
// The step is latency-bound at realistic batch sizes (a few pairs per lane over the whole chip), so
// a chunk is a short dependent chain  descriptor -> pair fields -> partner rows:
//   * the pair fields of the WHOLE chunk are fetched up front (lane t takes pairs t, t+LPR, ...,
//     coalesced) and staged in LDS; every trip reads the fields of its U pairs back with
//     ds_read_b128 (a broadcast inside the group);
//   * after that every trip costs one memory round trip with U partner rows in flight per group;
//   * groups are 8 lanes wide at d <= 64 (8 lanes x 2 float4 = one 128-B line per load), so a wave
//     carries 8 chunks and the per-pair bookkeeping (addresses, DPP butterfly, diff, e) is issued
//     once for 8 pairs;
//   * chunks are dealt to groups round-robin over the side's blocks so the full-length chunks of the
//     Zipf head do not pile up in a few workgroups.
// Measured in-process (tools/ab_kernels.py) against earlier forms: a wave per chunk (-40 %), per-pair
// ds_bpermute broadcasts on 16-lane groups (-7 % at B = 131072, -20 % at B = 1048576, d = 64).
// kChunkMax bounds chunk_cap.
// ------------------------------------------------------------------------------------------
constexpr int kChunkMax = 32;
constexpr int kFieldStride = kChunkMax + 4;      // dwords; +16 B staggers the groups over the LDS banks

// partner rows in flight per group, and the occupancy the register allocator is held to.  With both sides
// in one launch the grid at B = 131072, d = 64 is ~3700 waves: U = 4 + 4 waves/SIMD keeps all of them
// resident at once (A/B in-process: 12.1 us vs 13.8 us for U = 8 at 2 waves/SIMD; 42.9 vs 45.5 us at B = 1 M).
__device__ inline int grp_of(int tid, int lpr) { return tid / lpr; }

template <int NV> struct PassUnroll { static constexpr int value = NV == 1 ? 8 : 4; };
template <int LPR> struct PassWaves { static constexpr int value = LPR == 8 ? 4 : 1; };

struct PassSide {
    const int32_t *partner;        // [B] id of the other side's row, this side's sorted order
    const float *w, *y;            // [B] glove_weight / glove_value in the same order
    const int32_t *chunk_id, *chunk_start;
    const float *own, *other;      // own table (rows of this side's ids) / partner table
    const float *own_bias, *other_bias;
    float *gp, *gb;                // per-chunk partial gradient rows / bias gradients of this side
    float *e_out;                  // optional [B]: e_i in this side's order (row side: diagnostics, eval)
    int n_host;                    // chunks of this side if known on the host, else -1
    int count_index;               // counts[0] (row) or counts[2] (col)
    float *mark;                   // if not null: mark[id] = 1 for every id of this side (fused Adam step)
    const int32_t *crec;           // per-chunk records {id, n, first pair, only chunk of its id | partner | w | y} or nullptr
    const uint32_t *chunk_hw;      // without records: per chunk, (first chunk of its id) << 31 | chunks of the id behind it, or nullptr
    int capP;                      // chunk_cap rounded up to a multiple of 8 (record field length)
    // fused Adagrad apply (FUSE kernels): a chunk that is its id's ONLY chunk holds the id's whole gradient in
    // registers, next to the id's own row, so the update is formed here instead of travelling through a partial
    // row: the accumulator is updated in place (nobody else reads it), the new row goes
    //   fuse == kFuseInPlace  into the table (only legal when no concurrent work reads this side's table as partner
    //                         rows: the col side in a launch of its own, after the row side)
    //   fuse == kFuseSlot     into the chunk's partial-row slot (gp / gb), from where the apply kernel copies it
    //                         into the table once every pass that gathers the old rows has finished
    // fuse == kFuseNone: every chunk stores its partial sums (the apply / dense-gradient kernels do the rest)
    //   fuse == kFuseTwin     into the OTHER copy of a twinned table (glove_tables.R_ver: rows V_row .. 2 V_row - 1 are a
    //                         second copy of the row table, own_ver[u] says which copy of row u is current): later passes
    //                         of the step keep finding the old row in the current copy, the apply kernel only flips
    //                         own_ver[u] — no slot round trip, no copy
    int fuse;
    float *own_out, *own_bias_out; // this side's table / bias vector, written by kFuseInPlace / kFuseTwin
    float *S1, *S1b;               // this side's Adagrad accumulators
    const uint8_t *own_ver, *other_ver;   // not null: that table is twinned, ver[id] != 0 = the current row is id + twin rows
    int own_twin, other_twin;             // rows between the two copies (V_row)
    //   fuse == kFusePack     nothing is applied: the id's summed gradient (incl. the activity-L2 term) goes straight into
    //                         its entry of a packed list (glove_pack_grad_f32's layout) — the multi-GPU forms, whose
    //                         gradients travel before anything is applied; the pack launch then only adds the other ids
    //                         (no fields of their own — the struct is held in scalar registers, which are short: the list
    //                         is passed in own_out, the number of entries in front of this side's in own_twin)
};

constexpr int kFuseNone = 0, kFuseSlot = 1, kFuseInPlace = 2, kFuseTwin = 3, kFusePack = 4;

struct StepConsts {
    float kappa, kappa_b;       // 2 m l2 inv_batch / d , 2 m l2 inv_batch
    float lr, eps;
    float l2, m, inv_batch, inv_d;
};

// FUSE == 1: the accumulator row a whole run is going to need is requested when the run starts (it arrives under the
// partner-row trips) and waits in LDS, written there by the load itself (global_load_lds_dwordx4: no VGPRs held across
// the trips; the image is [k][lane of the wave], which is the order that instruction writes).  Kept in registers instead
// (NV float4 more per lane) the d = 300 shape spills at 3 waves per SIMD (measured variants).
// FUSE kernels keep the accumulator row of a run in registers as well: held to 3 waves per SIMD (168 VGPRs), which the
// d = 300 shape misses by one register otherwise
// FUSE: 0 classic schedule, 1 run-merged and applying (kFuseSlot / kFuseInPlace / kFuseTwin), 2 run-merged and packing
// (kFusePack) — a build of its own: the apply code and its accumulator rows would cost the other their registers
// Run-merged passes over rows of ONE float4 per lane (d = 128: 512-byte rows, bound by requests in flight, not by bytes): four
// partner rows per trip at four waves per SIMD (<= 128 VGPRs; 114 - 121 as built, nothing spilled) instead of eight at three —
// most chunks of a big batch hold one to three pairs, so half of an eight-row trip's loads were repeats of the chunk's first
// partner, and the fourth wave hides more of every trip than the second half of the trip did.  One process, same resident plans
// (tools/ab_kernels.py, V = 2 M, d = 128, B = 1 M, twin form): 505 -> 407 us per step, bit-identical tables; five waves spill
// (815 us), eight rows at four waves spill (1,088).  Three float4 per lane (d = 300) stay at four rows and three waves: two rows
// at four waves (128 VGPRs, nothing spilled) measured 610 against 582 us at V = 400 k and 107 against 97 at V = 50 k; four rows
// at four waves (compiled for one head: 165 VGPRs at three waves, 16 spilled at four) 697 against 574 and 122 against 95.
// (the run-merged passes of 8-lane groups without records — d <= 64 on vocabularies far beyond text8's: off the benchmarked
// path — do not fit four waves any more: three asked for, nothing spilled)
// (... and with the loss head read at run time — HEAD below: the logistic heads' exp / log expansions — the run-merged passes of
// 8-lane groups do not fit four waves with records either: 29 - 34 VGPRs spilled at 128; three asked for)
// (... and neither do their builds with solid workgroups — SOLID below: 2 VGPRs spilled at four waves)
template <int LPR, int NV, int FUSE, bool REC = true, int HEAD = 0, bool SOLID = false> struct FusePass {
    static constexpr bool narrow = FUSE != 0 && LPR != 8 && NV == 1;
    static constexpr int unroll = narrow ? 4 : PassUnroll<NV>::value;
    static constexpr int waves = narrow ? 4 : (FUSE != 0 && NV <= 3 && (LPR != 8 || !REC || HEAD < 0 || SOLID)) ? 3 : PassWaves<LPR>::value;
};
// HEAD: -1 = the loss head is read from the `head` argument at run time (the logistic heads); 0 = compiled for
// GLOVE_HEAD_REGRESSION (every pass of the GloVe estimator: the logistic epilogue's exp / log expansions cost the
// regression build 18 VGPRs at one float4 per lane — 119 against 101 — and 26 spilled scalar registers, whether they run or
// not.  V = 2 M, d = 128, B = 1 M on the same plans, one process: 397 -> 355 us per step; V = 400 k, d = 300: 562 -> 554)
// SIDE: -1 / -2 = the launch holds both sides (row side in the first row_blocks workgroups; -2: the twin form's launches on row
// tables of 128 MB and more, with the streaming cache policy below); 1 / 0 = it holds the row / the col side
// alone (the three-launch fused form's launches, and the twin form's on tables the caches hold; the col-side launch of the twin
// form — SIDE 0 or -2 — may carry the list tail): the col side's build then drops what only the loss needs — |c|^2 of every
// partner row (a fifth of a trip's arithmetic), the bias squares, e . diff — and with them 17 - 27 VGPRs (d = 300: 126 against
// 153: a fourth wave per SIMD).
// The twin form's col-side launch carries, behind its pass workgroups, the workgroups that list the light ids the apply launch
// still has to visit (a thread per distinct id: an id one run did not hold completely goes onto work[4 ...], work[0] counts
// them — zeroed by the row-side launch before).  The list depends on the plan alone, so it is drawn in the shadow of the pass's
// last workgroups instead of in a launch of its own between pass and apply (triage_kernel: 5 us + a launch boundary per step;
// the version flips of the finished row ids, which do have to wait for the col side's gathers, moved into the apply launch).
struct ListTail {
    const int32_t *counts;          // device counts[8]
    const int32_t *rec_r, *rec_c;   // {id, first chunk, chunks, pairs} per distinct id
    int nu_r_host, nu_c_host;       // -1 = read the device counts
    int heavy_chunks, per;
    int first_block;                // workgroups from here on list; < 0: no tail in this launch
};

__device__ inline void list_unfinished_ids(const ListTail &tl, int32_t *__restrict__ work, int q)
{
    const int nu_r = tl.nu_r_host >= 0 ? tl.nu_r_host : tl.counts[1];
    const int nu_c = tl.nu_c_host >= 0 ? tl.nu_c_host : tl.counts[3];
    if (q >= nu_r + nu_c) return;
    const int4 rec = q < nu_r ? reinterpret_cast<const int4 *>(tl.rec_r)[q] : reinterpret_cast<const int4 *>(tl.rec_c)[q - nu_r];
    if (rec.z > tl.heavy_chunks) return;                                            // heavy ids keep their own workgroups
    const int runs = 1 + (rec.y + rec.z - 1) / tl.per - rec.y / tl.per;             // (Slots::count)
    if (runs == 1) return;                                                          // one run held it: the pass applied it
    work[4 + atomicAdd(work, 1)] = q;
}

// SOLID: the build that adds up, per workgroup, the sums of lane groups that all hold one id (batches of 131,072 chunks a side and
// more: solid_groups) — a build of its own, so that the others keep their registers (compiled into all of them the epilogue cost
// five shapes a wave per SIMD and the 8-lane shapes 45 spilled VGPRs)
template <int LPR, int NV, bool FULL, bool REC, int FUSE, int HEAD = -1, int SIDE = -1, bool SOLID = false>
__global__ __launch_bounds__(kBlock, (FusePass<LPR, NV, FUSE, REC, HEAD, SOLID>::waves)) void sidepass_kernel(
    const int32_t *__restrict__ counts, PassSide rowside, PassSide colside, int row_blocks,
    const float *__restrict__ scalars, int64_t *__restrict__ step, int d4, float inv_batch,
    float *__restrict__ blockpart, int head, float neg_factor, StepConsts kc, int per, int32_t *__restrict__ work, ListTail tail)
{
    if (FUSE == 1 && (SIDE == -2 || SIDE == 0) && tail.first_block >= 0 && (int)blockIdx.x >= tail.first_block) {      // (block-uniform)
        list_unfinished_ids(tail, work, ((int)blockIdx.x - tail.first_block) * kBlock + (int)threadIdx.x);
        return;
    }
    constexpr int GPB = kBlock / LPR;
    constexpr int U = FusePass<LPR, NV, FUSE>::unroll;
    constexpr int SL = kChunkMax / LPR > 0 ? kChunkMax / LPR : 1;     // pairs a lane stages
    static_assert(U % 4 == 0 && U <= kRecPad && kRecPad % U == 0, "fields are read back four pairs at a time; record fields are padded to kRecPad slots");
    // [group][field][pair]: 0 partner, 1 w (REC) or w2 = 2 w inv_batch, 2 y.  With records the group's LDS image
    // is the record itself: header float4, then the blocks of 8 pairs (glove_common.h)
    constexpr int kRecStride = 4 + 3 * kChunkMax + 4;        // dwords; +16 B staggers the groups over the banks
    static_assert(kChunkMax % kRecPad == 0 && 4 + 3 * kChunkMax <= kRecStride, "the largest record fits a group's LDS image");
    __shared__ __attribute__((aligned(16))) uint32_t fld_raw[GPB * (REC ? kRecStride : 3 * kFieldStride)];
    uint32_t(*fld)[3][kFieldStride] = reinterpret_cast<uint32_t(*)[3][kFieldStride]>(fld_raw);
    uint32_t *rec = fld_raw + grp_of(threadIdx.x, LPR) * kRecStride;
    constexpr bool kPark = FUSE == 1;
    __shared__ __attribute__((aligned(16))) f4 park_raw[kPark ? (kBlock / 64) * NV * 64 : 1];
    f4 *park = park_raw + (kPark ? (threadIdx.x / 64) * NV * 64 : 0);       // this wave's image
    const int lg = threadIdx.x % LPR;
    const int grp = threadIdx.x / LPR;
    const bool is_row = SIDE < 0 ? (int)blockIdx.x < row_blocks : SIDE == 1;
    const PassSide &sd = is_row ? rowside : colside;
    const int bid = is_row ? blockIdx.x : blockIdx.x - row_blocks;
    const int nblk = is_row ? row_blocks : (FUSE == 1 && (SIDE == -2 || SIDE == 0) && tail.first_block >= 0 ? tail.first_block : (int)gridDim.x) - row_blocks;
    GLOVE_STAMP(0);
    const int n_chunks = sd.n_host >= 0 ? sd.n_host : counts[sd.count_index];
    const float g = scalars[0];
    // SIDE == -2: the twin form's launches — tables beyond the caches: the streams of a fused pass leave the L2 to the partner
    // rows (see "cache policy of the run-merged passes" above).  A build of its own: on cache-resident tables (V = 50 k, d = 300:
    // the three-launch form) the policy costs 8 % (94.0 -> 101.8 us per step: the next launch finds the finished rows in the caches
    // there), and as a run-time switch it cost every shape 1.2 %.
    constexpr bool streams = FUSE == 1 && SIDE == -2;
    if (is_row && blockIdx.x == 0 && threadIdx.x == 0) {
        *step += 1;                         // global_step (see glove_hip.h)
        if (FUSE && work) work[0] = 0;      // the apply side's work list starts empty (triage_kernel)
    }

    // loss partials (row side only): [0] sum e diff (= 2 inv_batch sum w diff^2), [1] sum |r|^2+|c|^2,
    // [2] sum b^2, [3] sum e
    float part[kPartials] = {0.f, 0.f, 0.f, 0.f};

    // Chunk schedule.
    //   classic: group (bid, grp) takes chunks bid*GPB+grp, += nblk*GPB; every chunk stores its own partial row.
    //   FUSE:    group number gq = bid*GPB+grp owns the `per` CONSECUTIVE chunks [gq*per, (gq+1)*per).  Chunks are sorted
    //            by id, so the group meets its ids as runs of consecutive chunks: the own row is loaded once per run, the
    //            gradient keeps accumulating in registers across the run's chunks (pairs in plan order), and a run that
    //            holds ALL chunks of its id is applied right here (sd.fuse); any other run stores ONE partial row, in the
    //            slot of its first chunk.  The apply kernel derives the same runs from (first chunk, chunks, per).
    int j = FUSE ? (bid * GPB + grp) * per : bid * GPB + grp;
    const int j_end = FUSE ? (j + per < n_chunks ? j + per : n_chunks) : n_chunks;
    const int j_step = FUSE ? 1 : nblk * GPB;
    // A plan without records (FUSE, run words): the descriptors of ALL the group's chunks — start, id, run word: 12 B each from
    // three arrays — arrive in one round trip up front and wait in LDS; a chunk then costs what a record costs: one trip for its
    // pair fields, then its partner rows.  (Fetched chunk by chunk they were a third dependent trip: 599 against 584 us per C4 step.)
    constexpr bool kDesc = FUSE == 1 && !REC;
    constexpr int kDescSlots = 16;
    __shared__ int32_t desc_raw[kDesc ? GPB * 4 * kDescSlots : 1];
    int32_t *desc = desc_raw + (kDesc ? grp * 4 * kDescSlots : 0);
    const bool use_desc = kDesc && sd.chunk_hw != nullptr && per < kDescSlots;
    const int j_first = j;
    // ... and the pair fields of all its chunks are ONE contiguous range of the side's arrays (a few dozen pairs for the short
    // chunks of a big batch): when they fit the group's stage they come in a second trip, coalesced, and the chunks take them
    // from LDS — no memory trip per chunk but its partner rows.  A longer range (the full chunks of the Zipf head) is read
    // chunk by chunk.
    constexpr int kStagePairs = 4 * LPR;        // 12 KB of LDS per workgroup at every shape
    __shared__ uint32_t stage_raw[kDesc ? GPB * 3 * kStagePairs : 1];
    uint32_t *stage = stage_raw + (kDesc ? grp * 3 * kStagePairs : 0);
    int stage_first = 0;
    bool staged = false;
    if (use_desc && j < j_end) {
        for (int x = lg; x <= j_end - j; x += LPR) {                 // (a group of 8 lanes owns up to 12 chunks: two rounds)
            desc[x] = sd.chunk_start[j + x];
            if (x < j_end - j) {
                const int32_t cid = sd.chunk_id[j + x];
                desc[kDescSlots + x] = cid;
                desc[2 * kDescSlots + x] = (int32_t)sd.chunk_hw[j + x];
                // twinned own table: which copy of the chunk's row is current, looked up here — behind the id, beside the pair
                // fields' trip — instead of as a dependent trip in front of every run's own-row load
                if (sd.own_ver) desc[3 * kDescSlots + x] = sd.own_ver[cid];
            }
        }
        stage_first = desc[0];
        const int span = desc[j_end - j] - stage_first;
        staged = span <= kStagePairs;
        if (staged) {
            for (int i = lg; i < span; i += LPR) {
                uint32_t pid = (uint32_t)sd.partner[stage_first + i];
                // twinned partner table: the staged ids become the rows that are current, here, once for all the group's chunks
                // (one byte gather per pair behind the id's load) instead of a dependent trip in front of every chunk's rows
                if (sd.other_ver) pid += sd.other_ver[pid] ? (uint32_t)sd.other_twin : 0u;
                stage[i] = pid;
                stage[kStagePairs + i] = __float_as_uint(sd.w[stage_first + i]);
                stage[2 * kStagePairs + i] = __float_as_uint(sd.y[stage_first + i]);
            }
        }
    }
    // FUSE == 1: a workgroup all of whose chunks belong to ONE id (the head of a Zipf batch: its full chunks fill dozens of
    // workgroups) adds its groups' sums up before it leaves — one partial row per workgroup instead of one per group for the one
    // workgroup that has to sum them in the apply launch (its longest chain: V = 400 k, B = 1 M, the id of rank 1: 400 rows)
    bool solid = false;
    if (FUSE == 1 && SOLID) {
        const int f0 = bid * GPB * per, l0 = f0 + GPB * per - 1;
        if (l0 < n_chunks) {
            if (REC) {
                const uint4 *rq = reinterpret_cast<const uint4 *>(sd.crec);
                const size_t stride = rec_stride_q(sd.capP);
                solid = rq[(size_t)f0 * stride].x == rq[(size_t)l0 * stride].x;
            } else {
                solid = sd.chunk_id[f0] == sd.chunk_id[l0];
            }
        }
    }
    int32_t cur_u = -1, own_at = 0;
    int run_first = 0, run_pairs = 0, run_q = 0;
    bool run_whole = false;
    f4 r[NV], acc[NV], A[NV];
    float own_b = 0.f, bg = 0.f, Ab = 0.f, se = 0.f;
    (void)A; (void)Ab;

    bool pending = false;                   // FUSE: a run whose sums are still in registers
    for (;; j += j_step) {
        const bool have = j < j_end;
        int32_t u = -1;
        int s = 0, n = 0, uq = 0;           // uq (records only): position of the id among the side's distinct ids
        uint32_t hw = 0;                    // record header word 3: (first chunk of its id) << 31 | chunks of the id after this one
        const int capP = sd.capP;
        if (!have) {
        } else if (REC) {
            // the record (descriptor + pair fields) in contiguous 16-B loads -> LDS as is
            const int rq = 1 + 3 * capP / 4;                // float4 of the packed record (the LDS image)
            const uint4 *rp = reinterpret_cast<const uint4 *>(sd.crec) + (size_t)j * rec_stride_q(capP);   // line 0: header | block 0 | pad
            uint4 *lrec = reinterpret_cast<uint4 *>(rec);
            if (FUSE != 0 && NV >= 3) {
                // run-merged passes over wide rows (bound by bytes): header + first block of 8 pairs (112 B, one round
                // trip); a chunk of more pairs fetches its other blocks once the header has told how many (a second
                // round trip for the long chunks only) — the padding up to the cap, 3/4 of a record on average, is
                // never read.  Measured in one process against whole-record reads: V = 400 k, d = 300, B = 1 M
                // 574 vs 579 us per step; V = 2 M, d = 128 495.6 vs 492.6 (512-B rows: bound by requests in flight,
                // not by bytes — hence NV >= 3; again with records on lines of their own: 532.6 vs 527.2); V = 400 k at B = 131,072 139.0 vs 139.6
                constexpr int kHead = 1 + 6;
                static_assert(LPR >= kHead, "one load per lane covers the header and the first block");
                if (lg < kHead) lrec[lg] = rp[lg];
                const int n1 = (int)lrec[0].y;
                const int nq = 1 + 6 * ((n1 + kRecPad - 1) / kRecPad);
                for (int f = kHead + lg; f < nq; f += LPR) lrec[f] = rp[f + 1];     // blocks 1 ..: behind line 0's padding
            } else {
                // latency-bound forms: ONE round trip for the whole record
                for (int f = lg; f < rq; f += LPR) lrec[f] = rp[rec_gq(f)];
            }
            const uint4 hdr = lrec[0];          // same wave wrote it: LDS ops of one wave complete in order
            u = (int32_t)hdr.x;
            n = (int)hdr.y;
            uq = (int)hdr.z;
            hw = hdr.w;
            GLOVE_DRAIN(); GLOVE_STAMP(1);
        } else {
            if (use_desc) {                     // (same wave wrote them: LDS ops of one wave complete in order)
                const int x = j - j_first;
                s = desc[x];
                n = desc[x + 1] - s;
                u = desc[kDescSlots + x];
                hw = (uint32_t)desc[2 * kDescSlots + x];
            } else {
                u = sd.chunk_id[j];
                s = sd.chunk_start[j];
                n = sd.chunk_start[j + 1] - s;
                if (FUSE && sd.chunk_hw) hw = sd.chunk_hw[j];       // (a plan without records that carries its run words: glove_plan.r_chunk_hw)
            }
            GLOVE_DRAIN(); GLOVE_STAMP(1);      // descriptor arrived
#pragma unroll
            for (int sl = 0; sl < SL; ++sl) {
                const int t = lg + sl * LPR;
                int32_t pv;
                float wv, yv;
                if (kDesc && staged) {              // (the group's stage: same wave wrote it)
                    const int k = s - stage_first + (t < n ? t : 0);
                    pv = (int32_t)stage[k];
                    wv = __uint_as_float(stage[kStagePairs + k]);
                    yv = __uint_as_float(stage[2 * kStagePairs + k]);
                } else {
                    const int k = s + (t < n ? t : 0);
                    pv = sd.partner[k];
                    wv = sd.w[k];
                    yv = sd.y[k];
                }
                if (t < kChunkMax) {
                    fld[grp][0][t] = (uint32_t)pv;
                    fld[grp][1][t] = __float_as_uint(t < n ? wv : 0.f);     // tail slots weigh 0
                    fld[grp][2][t] = __float_as_uint(yv);
                }
            }
        }
        if (FUSE && have && sd.other_ver && !(kDesc && staged)) {      // (staged pairs were resolved when they were staged)
            // twinned partner table: the staged partner ids become the rows that are current.  One byte gather per pair,
            // issued with the own-row load below (whose latency covers it), instead of a dependent hop in every trip
            for (int t = lg; t < n; t += LPR) {
                uint32_t *slot = REC ? rec + rec_pair(t) : &fld[grp][0][t];
                const uint32_t id = *slot;
                *slot = id + (sd.other_ver[id] ? (uint32_t)sd.other_twin : 0u);
            }
        }
        const bool new_run = !FUSE || !pending || u != cur_u;
        if (FUSE && pending && (!have || new_run)) {        // the run in registers is complete
            pending = false;
            if (FUSE == 2 && run_whole) {
                // the id's whole gradient is here and it is wanted as a packed-list entry (PackGrad's arithmetic)
                const float cnt = (float)run_pairs;
                const float kcn = kc.kappa * cnt;
                float Gb = se;
#pragma unroll
                for (int k = 0; k < NV; ++k) acc[k] += kcn * r[k];
                Gb += kc.kappa_b * cnt * own_b;
                f4 *e = reinterpret_cast<f4 *>(sd.own_out) + (size_t)(sd.own_twin + run_q) * ((size_t)d4 + 1);
#pragma unroll
                for (int k = 0; k < NV; ++k) {
                    const int i4 = lg + k * LPR;
                    if (i4 < d4) e[i4] = acc[k];
                }
                if (lg == 0) e[d4] = f4{Gb, __int_as_float(cur_u), __int_as_float(is_row ? 0 : 1), 0.f};
            } else if (FUSE == 1 && run_whole) {
                // the id's whole gradient is here: G = sum + activity-L2 term, then Adagrad (the arithmetic of
                // for_each_id + AdagradApply; on an id with a single chunk expression for expression, bit-identical)
                const float cnt = (float)run_pairs;
                const float kcn = kc.kappa * cnt;
                float bval = own_b, Gb = se;
#pragma unroll
                for (int k = 0; k < NV; ++k) acc[k] += kcn * r[k];
                Gb += kc.kappa_b * cnt * bval;
                // every load of the run has been consumed by now, the parked row (requested before them) has landed
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
                for (int k = 0; k < NV; ++k) A[k] = park[k * 64 + (threadIdx.x & 63)];
#pragma unroll
                for (int k = 0; k < NV; ++k) adagrad_vec(r[k], A[k], acc[k], kc.lr, kc.eps);
                if (streams) store_row_wt<LPR, NV>(sd.S1, (size_t)cur_u, d4, lg, A); else store_row<LPR, NV>(sd.S1, (size_t)cur_u, d4, lg, A);
                const bool to_slot = sd.fuse == kFuseSlot;
                // in place: the row itself; twin: the copy that is NOT current (own_at is the current one)
                const size_t out_at = sd.fuse == kFuseTwin ? (size_t)(own_at == cur_u ? cur_u + sd.own_twin : cur_u) : (size_t)cur_u;
                if (streams) store_row_wt<LPR, NV>(to_slot ? sd.gp : sd.own_out, to_slot ? (size_t)run_first : out_at, d4, lg, r);
                else store_row<LPR, NV>(to_slot ? sd.gp : sd.own_out, to_slot ? (size_t)run_first : out_at, d4, lg, r);
                if (lg == 0) {
                    adagrad_elem(bval, Ab, Gb, kc.lr, kc.eps);
                    sd.S1b[cur_u] = Ab;
                    if (to_slot) sd.gb[run_first] = bval; else sd.own_bias_out[out_at] = bval;
                }
            } else if (!(FUSE == 1 && SOLID && solid)) {     // (a solid workgroup's sums leave together, below)
                store_row<LPR, NV>(sd.gp, (size_t)run_first, d4, lg, acc);
                if (lg == 0) {
                    sd.gb[run_first] = se;
                    if (FUSE == 0 && sd.mark) sd.mark[cur_u] = 1.0f;
                }
            }
        }
        if (!have) break;
        if (new_run) {
            cur_u = u;
            run_first = j;
            run_q = uq;
            run_pairs = 0;
            own_at = u;
            if (FUSE && sd.own_ver)                                                     // the current copy of a twinned table
                own_at = u + ((use_desc ? desc[3 * kDescSlots + (j - j_first)] : (int32_t)sd.own_ver[u]) ? sd.own_twin : 0);
            if (FUSE && streams) load_row_nt<LPR, NV>(r, sd.own, own_at, d4, lg);
            else if (FUSE) load_row<LPR, NV>(r, sd.own, own_at, d4, lg);
            else load_row<LPR, NV>(r, sd.own, u, d4, lg);
            own_b = sd.own_bias[own_at];
            bg = own_b + g;
            // whole: the run starts at the id's first chunk and the id's last chunk is still inside this group's range
            run_whole = FUSE && sd.fuse != kFuseNone && (hw >> 31) != 0 && j + (int)(hw & 0x7fffffffu) < j_end;
            if (FUSE == 1 && run_whole) {   // requested with the own row: arrives under the partner-row trips
                const f4 *src = reinterpret_cast<const f4 *>(sd.S1) + (size_t)u * d4;
#pragma unroll
                for (int k = 0; k < NV; ++k) {
                    const int i4 = lg + k * LPR;
                    // destination: the wave-uniform base + lane * 16 B (the hardware adds the lane part)
                    if (!(FULL || i4 < d4)) continue;
                    if (streams) __builtin_amdgcn_global_load_lds(src + i4, (__attribute__((address_space(3))) void *)(park + k * 64), 16, 0, 2);      // aux 2 = nt
                    else __builtin_amdgcn_global_load_lds(src + i4, (__attribute__((address_space(3))) void *)(park + k * 64), 16, 0, 0);
                }
                Ab = sd.S1b[u];
            }
#pragma unroll
            for (int k = 0; k < NV; ++k) acc[k] = f4{0.f, 0.f, 0.f, 0.f};
            se = 0.f;
        }
        run_pairs += n;
        float se_c = 0.f, cc_sum = 0.f, bsq = 0.f, ed = 0.f;
        GLOVE_DRAIN(); GLOVE_STAMP(2);      // pair fields staged, own row arrived
        // fields written by this wave's own lanes: LDS ops of one wave complete in order

        for (int q0 = 0; q0 < n; q0 += U) {
            int32_t col[U];
            float w2[U], yq[U];
#pragma unroll
            for (int a4 = 0; a4 < U; a4 += 4) {
                const int rp0 = rec_pair(q0 + a4);          // records: blocks of 8 pairs {partner | w | y}
                const uint4 pc = *reinterpret_cast<const uint4 *>(REC ? &rec[rp0] : &fld[grp][0][q0 + a4]);
                const uint4 pw = *reinterpret_cast<const uint4 *>(REC ? &rec[rp0 + kRecPad] : &fld[grp][1][q0 + a4]);
                const uint4 py = *reinterpret_cast<const uint4 *>(REC ? &rec[rp0 + 2 * kRecPad] : &fld[grp][2][q0 + a4]);
                col[a4] = (int32_t)pc.x; col[a4 + 1] = (int32_t)pc.y; col[a4 + 2] = (int32_t)pc.z; col[a4 + 3] = (int32_t)pc.w;
                const float sc2 = 2.0f * inv_batch;
                w2[a4] = sc2 * __uint_as_float(pw.x); w2[a4 + 1] = sc2 * __uint_as_float(pw.y);
                w2[a4 + 2] = sc2 * __uint_as_float(pw.z); w2[a4 + 3] = sc2 * __uint_as_float(pw.w);
                yq[a4] = __uint_as_float(py.x); yq[a4 + 1] = __uint_as_float(py.y);
                yq[a4 + 2] = __uint_as_float(py.z); yq[a4 + 3] = __uint_as_float(py.w);
            }
            f4 c[U][NV];
            float bcv[U];
#pragma unroll
            for (int a = 0; a < U; ++a) {
                load_row_fast<LPR, NV, FULL>(c[a], sd.other, col[a], d4, lg);
                // the partner bias enters the dot once, through lane 0 of the group (a masked 1-lane-per-group
                // load instead of a 64-lane gather of the same 4 bytes), and the butterfly spreads it
                bcv[a] = 0.f;
                if (lg == 0) bcv[a] = *reinterpret_cast<const float *>(reinterpret_cast<const char *>(sd.other_bias) + (uint32_t)col[a] * 4u);
            }
            float dp[U], cc[U];
#pragma unroll
            for (int a = 0; a < U; ++a) {
                dp[a] = 0.f; cc[a] = 0.f;
#pragma unroll
                for (int k = 0; k < NV; ++k) { dp[a] += dot4(r[k], c[a][k]); cc[a] += dot4(c[a][k], c[a][k]); }
                dp[a] += bcv[a];                                     // non-zero in lane 0 only
            }
            // the U butterflies are independent: stage by stage so the DPP hazards overlap
#pragma unroll
            for (int a = 0; a < U; ++a) dp[a] = dpp_add<0xB1>(dp[a]);
#pragma unroll
            for (int a = 0; a < U; ++a) dp[a] = dpp_add<0x4E>(dp[a]);
#pragma unroll
            for (int a = 0; a < U; ++a) dp[a] = dpp_add<0x141>(dp[a]);
            if (LPR >= 16) {
#pragma unroll
                for (int a = 0; a < U; ++a) dp[a] = dpp_add<0x140>(dp[a]);
            }
            if (LPR >= 32) {
#pragma unroll
                for (int a = 0; a < U; ++a) dp[a] += __shfl_xor(dp[a], 16, 64);
            }
            if (LPR >= 64) {
#pragma unroll
                for (int a = 0; a < U; ++a) dp[a] += __shfl_xor(dp[a], 32, 64);
            }
            float ev[U];
#pragma unroll
            for (int a = 0; a < U; ++a) {
                const float valid = (q0 + a < n) ? 1.0f : 0.f;
                float e;
                if (HEAD == GLOVE_HEAD_REGRESSION || (HEAD < 0 && head == GLOVE_HEAD_REGRESSION)) {                 // uniform branch
                    float logit = dp[a] + bg;
                    asm("" : "+v"(logit));                          // (the logit, the difference and e: each a rounded value of its own in
                    float diff = logit - yq[a];                     // every build — see below)
                    asm("" : "+v"(diff));
                    e = w2[a] * diff;                               // 0 on tail slots
                    // (e is a rounded product for every consumer, as it is where the head is a run-time branch and e leaves it
                    // through a select: compiled for one head the sum of e's below would otherwise contract into fma(w2, diff, .)
                    // and the builds would differ in the last bit of the bias gradients)
                    asm("" : "+v"(e));
                    ed += e * diff;
                } else {
                    // pos / neg logistic heads on one logit: dL/dp = (pos (s - 1) + nf neg s) / B, s = sigmoid(p);
                    // `ed` collects 2/B times the pair's loss so that the common rescaling below applies
                    const float p = dp[a] + bg;
                    const float en = expf(-fabsf(p));               // in (0, 1]: no overflow either way
                    const float s = (p >= 0.f ? 1.0f : en) / (1.0f + en);
                    const float lse = log1pf(en);                   // softplus(x) = max(x, 0) + log1p(exp(-|x|))
                    const float wn = 2.0f * inv_batch * neg_factor * valid * yq[a];
                    e = 0.5f * (w2[a] * (s - 1.0f) + wn * s);
                    ed += w2[a] * (fmaxf(-p, 0.f) + lse) + wn * (fmaxf(p, 0.f) + lse);
                }
#pragma unroll
                for (int k = 0; k < NV; ++k) acc[k] += e * c[a][k];
                se_c += e;
                cc_sum += valid * cc[a];
                bsq += valid * bcv[a] * bcv[a];
                ev[a] = e;
            }
            if (FUSE == 0 && !REC && sd.e_out) {                  // glove_rowpass_f32 only (classic schedule): e_i for diagnostics
                constexpr int ES = (U + LPR - 1) / LPR;      // pairs of this trip whose e a lane stores
#pragma unroll
                for (int x = 0; x < ES; ++x) {
                    float mine = 0.f;
#pragma unroll
                    for (int a = x * LPR; a < U && a < (x + 1) * LPR; ++a) mine = (lg == a - x * LPR) ? ev[a] : mine;
                    const int q = q0 + lg + x * LPR;
                    if (lg + x * LPR < U && q < n) sd.e_out[s + q] = mine;
                }
            }
        }
        GLOVE_STAMP(3);                     // all partner-row trips issued and consumed
        se += se_c;
        if (is_row) {
            float rr = 0.f;
#pragma unroll
            for (int k = 0; k < NV; ++k) rr += dot4(r[k], r[k]);
            part[1] += cc_sum + (float)n * rr;
            if (lg == 0) {
                part[0] += ed;
                part[2] += bsq + (float)n * own_b * own_b;
                part[3] += se_c;
            }
        }
        if (FUSE) {
            pending = true;
        } else {
            store_row<LPR, NV>(sd.gp, (size_t)j, d4, lg, acc);
            if (lg == 0) {
                sd.gb[j] = se;
                if (sd.mark) sd.mark[u] = 1.0f;
            }
        }
    }
    if (FUSE == 1 && SOLID && solid) {      // block-uniform
        // every group holds the sums of its one run (same id everywhere): groups 0 .. GPB - 1 added in that order by group 0, one
        // partial row in the slot of the workgroup's first chunk.  (A wave writes into its own part of the parking image, which
        // no run of a solid workgroup has used: no run of it was whole.)
        __shared__ float solid_bias[SOLID ? GPB : 1];
        f4 *sums = park_raw;
#pragma unroll
        for (int k = 0; k < NV; ++k) sums[(grp * NV + k) * LPR + lg] = acc[k];
        if (lg == 0) solid_bias[grp] = se;
        __syncthreads();
        if (grp == 0) {
#pragma unroll 1
            for (int g2 = 1; g2 < GPB; ++g2) {
#pragma unroll
                for (int k = 0; k < NV; ++k) acc[k] += sums[(g2 * NV + k) * LPR + lg];
                se += solid_bias[g2];
            }
            const size_t slot = (size_t)bid * GPB * per;
            store_row<LPR, NV>(sd.gp, slot, d4, lg, acc);
            if (lg == 0) sd.gb[slot] = se;
        }
    }
    GLOVE_DRAIN(); GLOVE_STAMP(4);          // stores retired
    if (is_row) {                           // block-uniform
        part[0] *= 0.5f / inv_batch;        // sum e diff = 2 inv_batch sum w diff^2
        block_partials_store(part, blockpart);
    }
    GLOVE_DRAIN(); GLOVE_STAMP(5);
}

// ... and a run-time condition (rows that fill their lanes: LPR * NV == d4 -> FULL) as a compile-time bool
template <class F>
static void dispatch_bool(bool on, F f)
{
    if (on) f(std::true_type{}); else f(std::false_type{});
}


// One call on the step path: its arguments, validated once by the entry point that opens it (open_call, glove_step.hip), and
// what every launcher behind it would otherwise derive from them again
struct StepCall {
    const glove_plan *p;
    const glove_tables *t;
    const glove_hyper *h;
    void *ws;
    size_t ws_bytes;
    hipStream_t st;
    StepWs w;                   // the workspace, carved
    int d4;
    RowShape shape, pass;       // pick_row_shape / pick_pass_shape of d4
    int sides;                  // glove_hyper.sides: 1 rows, 2 cols, 3 both
    StepConsts k;
};

// What launch_passes (glove_step.hip) has worked out, as the objects that hold sidepass_kernel's builds take it
struct PassLaunch {
    const StepCall &c;
    PassSide rs, cs;
    ListTail tail;
    int per, row_blocks, nb, nb_launch, which;
    bool twin, solid, streaming, rec, pack, fuse;
};

// The launch of sidepass_kernel's builds for the shapes <LA, NA> and <LB, NB>: the object that calls it holds them, and no other may
template <int LA, int NA, int LB, int NB>
static int launch_pass_shapes(const PassLaunch &a)
{
    static_assert(pass_shape_listed(RowShape{LA, NA}) && pass_shape_listed(RowShape{LB, NB}), "only shapes pick_pass_shape selects are built");
    const glove_plan *p = a.c.p;
    const glove_tables *t = a.c.t;
    const glove_hyper *h = a.c.h;
    const PassSide &rs = a.rs, &cs = a.cs;
    const StepWs &w = a.c.w;
    const StepConsts &kc = a.c.k;
    const ListTail &tail = a.tail;
    const int d4 = a.c.d4, per = a.per, row_blocks = a.row_blocks, nb = a.nb, nb_launch = a.nb_launch, which = a.which;
    const bool twin = a.twin, solid = a.solid, streaming = a.streaming, rec = a.rec, pack = a.pack, fuse = a.fuse;
    hipStream_t st = a.c.st;
#define ARGS p->counts, rs, cs, row_blocks, t->scalars, t->step, d4, h->inv_batch, w.blockpart, (int)h->head, h->neg_factor, kc, per, w.work, tail
// (K: one launch of the build <..., HEAD, SIDE>, in its solid form where the batch calls for it — FUSE == 1 only)
#define K(LPR, NV, FULL, REC, FUSE, HEAD, SIDE, GRID)                                                                          \
    do {                                                                                                                       \
        if (FUSE == 1 && solid)                                                                                                \
            hipLaunchKernelGGL((sidepass_kernel<LPR, NV, FULL, REC, FUSE, HEAD, SIDE, FUSE == 1>), dim3(GRID), dim3(kBlock), 0, st, ARGS); \
        else                                                                                                                   \
            hipLaunchKernelGGL((sidepass_kernel<LPR, NV, FULL, REC, FUSE, HEAD, SIDE, false>), dim3(GRID), dim3(kBlock), 0, st, ARGS); \
    } while (0)
#define LAUNCH(LPR, NV, FULL, REC, FUSE)                                                                                       \
    do {                                                                                                                       \
        /* every pass compiled for the regression head (the same bits are asked of all of them on ids one chunk holds: one     \
         * epilogue, one set of contraction decisions); the logistic heads keep the run-time branch (compiled alone their      \
         * d = 300 build spills) */                                                                                             \
        /* (the side-specialised builds on tables the caches hold — three-launch form and twin form alike: there the col side's     \
         * fourth wave pays, V = 50 k, d = 300 96.8 -> 93.4 us per step; on tables beyond them, bound by bandwidth, it costs:        \
         * V = 400 k 577.6 -> 580.0, V = 2 M 361.5 -> 364.2) */ \
        if (h->head == GLOVE_HEAD_REGRESSION && FUSE == 1 && which == 1 && !(twin && streaming))                                \
            K(LPR, NV, FULL, REC, FUSE, GLOVE_HEAD_REGRESSION, (FUSE == 1 ? 1 : -1), nb);                                        \
        else if (h->head == GLOVE_HEAD_REGRESSION && FUSE == 1 && which == 2 && !(twin && streaming))                           \
            K(LPR, NV, FULL, REC, FUSE, GLOVE_HEAD_REGRESSION, (FUSE == 1 ? 0 : -1), nb_launch);                                 \
        else if (h->head == GLOVE_HEAD_REGRESSION && FUSE == 1 && twin)         /* (tables beyond the caches: the streaming build) */ \
            K(LPR, NV, FULL, REC, FUSE, GLOVE_HEAD_REGRESSION, (FUSE == 1 ? -2 : -1), nb_launch);                                \
        else if (h->head == GLOVE_HEAD_REGRESSION)                                                                              \
            K(LPR, NV, FULL, REC, FUSE, GLOVE_HEAD_REGRESSION, -1, nb);                                                          \
        else if (FUSE == 1 && twin)                  /* (the logistic heads: one twin build, streaming) */                      \
            K(LPR, NV, FULL, REC, FUSE, -1, (FUSE == 1 ? -2 : -1), nb_launch);                                                   \
        else                                                                                                                   \
            K(LPR, NV, FULL, REC, FUSE, -1, -1, nb);                                                                             \
    } while (0)
#define CALL(LPR, NV)                                                                   \
    dispatch_bool(LPR * NV == d4, [&](auto full) {                                      \
        constexpr bool FULL = decltype(full)::value;                                    \
        if (rec) { if (pack) LAUNCH(LPR, NV, FULL, true, 2); else if (fuse) LAUNCH(LPR, NV, FULL, true, 1); else LAUNCH(LPR, NV, FULL, true, 0); } \
        else { if (fuse) LAUNCH(LPR, NV, FULL, false, 1); else LAUNCH(LPR, NV, FULL, false, 0); }        \
    })
    if (a.c.pass.lpr == LA && a.c.pass.nv == NA) CALL(LA, NA);
    else if (a.c.pass.lpr == LB && a.c.pass.nv == NB) CALL(LB, NB);
    else return GLOVE_E_BADARG;
#undef CALL
#undef LAUNCH
#undef K
#undef ARGS
    return 0;
}

// (none of these leaves the library)
#pragma GCC visibility push(hidden)
int launch_passes_lpr8(const PassLaunch &a);        // glove_step_passes_lpr8.hip: <8, 1>, <8, 2>
int launch_passes_mid(const PassLaunch &a);         // glove_step_passes_mid.hip:  <32, 3>, <64, 2>
int launch_passes_wide(const PassLaunch &a);        // glove_step_passes_wide.hip: <64, 3>, <64, 4>
#ifdef GLOVE_STAMPS
int set_stamps_step(void *p);
int set_stamps_passes_lpr8(void *p);
int set_stamps_passes_mid(void *p);
int set_stamps_passes_wide(void *p);
#endif
#pragma GCC visibility pop

}  // namespace glove

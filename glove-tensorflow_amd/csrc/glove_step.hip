// GloVe training step on gfx950: fused forward + gradient passes and the optimizer applies.
//
// What the kernels replace (reference = /root/reference, TF graph built by model_fn):
//   rowpass   ResourceGather x4 + dot + Add (src/models/model_utils.py:41-54), weighted MSE head
//             (src/models/estimator.py:48-56), activity-L2 losses (model_utils.py:18-21,52) and
//             the row-side half of tf.gradients.
//   colpass   the col-side half of tf.gradients.
//   apply     OptimizerV2 dedup (Unique + UnsortedSegmentSum) + ResourceSparseApplyAdagradV2.
//   dense_*   the same sums written to dense [V,d] buffers (DP all-reduce), ResourceApplyAdagradV2
//             and Keras-legacy Adam (whole-table decay).
//
// Memory-bound gather/scatter: no MFMA.  A row of d floats is spread over LPR lanes as float4;
// a wave64 therefore works on 64/LPR chunks at once.  All sums have a fixed order, so a step is
// bitwise repeatable for a given plan.
#include "glove_step_passes.h"

namespace glove {

// ------------------------------------------------------------------------------------------
// Summed gradient of one distinct id: chunk partials in a fixed order + activity-L2 term.
// Light ids (at most plan.heavy_chunks chunks: almost all of them) are summed by one group of LPR
// lanes.  The ids of the Zipf head ("the", "<UNK>" own thousands of pairs of a large batch) are
// listed in plan.heavy; each gets a whole workgroup (the first `heavy_blocks` blocks of the grid, so
// they start ahead of the light work and run beside it): GPB groups stride over the partial rows,
// then group 0 adds the GPB sums in order.
// ------------------------------------------------------------------------------------------
struct SideBufs {
    const int32_t *uniq_rec;
    const float *gp, *gb;
    float *W, *S1, *bias, *S1b;
    uint8_t *ver;               // not null: W / bias are twinned (glove_tables.R_ver), ver[id] != 0 = current row is id + twin
    int twin;
};

// row of W / entry of bias that currently holds id (the slots S1 / S1b are never twinned)
__device__ inline int32_t cur_row(const SideBufs &sb, int32_t id) { return sb.ver && sb.ver[id] ? id + sb.twin : id; }

struct IdWork {
    const int32_t *counts;      // device counts[8]
    int nu_r_host, nu_c_host, n_heavy_host;   // host copies, -1 = read the device counts
    const int32_t *heavy;       // (side << 30) | q
    int heavy_blocks;           // leading blocks of the grid reserved for heavy ids
    int heavy_chunks;           // threshold
    int sides;                  // 1 = rows only, 2 = cols only, 3 = both
    int pre_r, pre_c;           // what a FUSE pass already did for the ids one run held completely (kFuse*), per side
    int per;                    // consecutive chunks per group of that FUSE pass
    int gpb;                    // ... and its lane groups per workgroup (solid workgroups leave one partial row: Slots); 0 = none
    const int32_t *work;        // not null: triage_kernel listed the light ids that still need this launch: work[0] = their
                                // number, work[4 ...] = their positions q (row ids first, col ids behind nu_r)
    int flips;                  // 1: the list came from the col-side launch (ListTail): the version flips of the row ids a run of the
                                // twin form's row pass finished are still to do — here, a thread per row id
};

// The partial rows of one id.  Classic passes: one per chunk, slots f .. f+n-1 (per == 1).  FUSE passes: one per run, a
// run being the id's chunks inside one group's range of `per` consecutive chunks: the k-th run starts at the id's
// first chunk (k == 0) or at the k-th multiple of `per` behind it.
// Behind a run-merged applying pass (gpb > 0: its lane groups per workgroup) a workgroup whose gpb * per chunks ALL belong to the
// id — a "solid" workgroup: the head of a Zipf batch owns dozens of them — has added its groups' sums up in LDS and left ONE
// partial row, in the slot of its first chunk (sidepass_kernel): the runs of the id are then the group ranges in front of its first
// solid workgroup, one per solid workgroup, and the group ranges behind the last (the id of rank 1 of the headline batch: 55 partial
// rows instead of 400 for the one workgroup that sums them in the apply launch).
struct Slots {
    int f, per, count;
    int gpb, g0, head, sb0, nsb;
    bool one_group;
    __device__ Slots(int first_chunk, int chunks, int per_, int gpb_ = 0) : f(first_chunk), per(per_), gpb(gpb_)
    {
        g0 = first_chunk / per_;
        const int g1 = (first_chunk + chunks - 1) / per_;
        one_group = g1 == g0;                                       // one group's range held all its chunks: the pass applied it
        count = head = 1 + g1 - g0;
        sb0 = nsb = 0;
        if (gpb_ > 0) {
            const int bc = gpb_ * per_;                             // chunks of a workgroup
            const int bs = (first_chunk + bc - 1) / bc;             // workgroups [bs, be) lie inside the id's chunks
            const int be = (first_chunk + chunks) / bc;
            if (be > bs) {
                sb0 = bs;
                nsb = be - bs;
                head = bs * gpb_ - g0;
                count = head + nsb + (g1 + 1 - be * gpb_);
            }
        }
    }
    __device__ int at(int k) const
    {
        if (k == 0) return f;
        if (k < head) return (g0 + k) * per;
        if (k < head + nsb) return (sb0 + (k - head)) * gpb * per;
        return ((sb0 + nsb) * gpb + (k - head - nsb)) * per;
    }
};

// G += partial rows k0, k0+stride, ... (< sl.count), PB loads in flight at a time, added in order
template <int LPR, int NV, int PB = 4>
__device__ inline void sum_partials(const SideBufs &sb, const Slots &sl, int k0, int stride, int d4, int lg,
                                    f4 (&G)[NV], float &Gb)
{
    for (int k = k0; k < sl.count; k += stride * PB) {
        f4 p[PB][NV];
        float pbias[PB];
#pragma unroll
        for (int a = 0; a < PB; ++a) {
            const int x = k + a * stride;
            const int xs = sl.at(x < sl.count ? x : 0);
            load_row<LPR, NV>(p[a], sb.gp, xs, d4, lg);
            pbias[a] = sb.gb[xs];
        }
#pragma unroll
        for (int a = 0; a < PB; ++a) {
            const float on = (k + a * stride < sl.count) ? 1.0f : 0.f;
#pragma unroll
            for (int kk = 0; kk < NV; ++kk) G[kk] += on * p[a][kk];
            Gb += on * pbias[a];
        }
    }
}

// Visits every distinct id of both sides once.  `fn` supplies
//   fn.prefetch(is_row, id, st)                     its own rows + bias slots (F::State: the Adagrad
//                                                   accumulator, Adam's m and v, or the dense gradient
//                                                   row), requested together with the table row so the
//                                                   latencies overlap
//   fn.finish(is_row, id, wid, q, G, Wv, Gb, bval, st)   G = summed gradient incl. the activity-L2 term; wid = row of
//                                                   the table that holds id (id itself unless the table is twinned); q = position of
//                                                   the id among its side's distinct ids (plan order)
// Returns true in the workgroup that should also do the once-per-step scalar work.
template <int LPR, int NV, class F>
__device__ inline bool for_each_id(const IdWork &wk, const SideBufs &rs, const SideBufs &cs,
                                   int d4, const StepConsts &k, F fn, int grid_blocks = 0)
{
    const int nblocks = grid_blocks > 0 ? grid_blocks : (int)gridDim.x;    // workgroups doing this traversal
    constexpr int GPB = kBlock / LPR;
    __shared__ f4 red[GPB][LPR * NV];
    __shared__ float redb[GPB];
    const int lg = threadIdx.x % LPR;
    const int grp = threadIdx.x / LPR;
    GLOVE_STAMP(0);

    if ((int)blockIdx.x < wk.heavy_blocks) {
        // ---- one heavy id for the whole workgroup
        const int n_heavy = wk.n_heavy_host >= 0 ? wk.n_heavy_host : wk.counts[4];
        if ((int)blockIdx.x >= n_heavy) return false;
        const int code = wk.heavy[blockIdx.x];
        const bool is_row = (code >> 30) == 0;
        if (!(wk.sides & (is_row ? 1 : 2))) return false;
        const SideBufs &sb = is_row ? rs : cs;
        const int4 rec = reinterpret_cast<const int4 *>(sb.uniq_rec)[code & 0x3fffffff];
        const int32_t id = rec.x;
        const int pre = is_row ? wk.pre_r : wk.pre_c;
        const Slots sl(rec.y, rec.z, pre != kFuseNone ? wk.per : 1, pre != kFuseNone ? wk.gpb : 0);
        if (pre != kFuseNone && sl.one_group) {       // one run held the whole id: the pass kernel applied it
            if (pre == kFuseSlot && grp == 0) {
                f4 Wn[NV];
                load_row<LPR, NV>(Wn, sb.gp, sl.f, d4, lg);
                const float bn = sb.gb[sl.f];
                store_row<LPR, NV>(sb.W, (size_t)id, d4, lg, Wn);
                if (lg == 0) sb.bias[id] = bn;
            }
            if (pre == kFuseTwin && threadIdx.x == 0) sb.ver[id] ^= 1;       // the other copy holds the new row
            return false;
        }
        const int32_t wid = cur_row(sb, id);
        f4 G[NV], Wv[NV];
        typename F::State st;
        float Gb = 0.f, bval = 0.f;
#pragma unroll
        for (int kk = 0; kk < NV; ++kk) G[kk] = f4{0.f, 0.f, 0.f, 0.f};
        if (grp == 0) {
            load_row<LPR, NV>(Wv, sb.W, wid, d4, lg);
            bval = sb.bias[wid];
            fn.prefetch(is_row, id, st);
        }
        // a heavy id is the longest dependent chain of the launch (the head of a Zipf batch: ~50 rows per group):
        // four rows in flight per trip at every row width (16 cost the d = 64 shape its occupancy: 8.4 -> 9.3 us; round 5, the
        // twin form's short-list apply, whole step, same plans: V = 400 k, d = 300 548.8 us with 4, 556.5 with 8, 555.4 with 16;
        // V = 2 M, d = 128 359.1 / 358.0 / 360.1 — profiles/r05_exp_heavy_rows_in_flight.txt)
        sum_partials<LPR, NV, 4>(sb, sl, grp, GPB, d4, lg, G, Gb);
#pragma unroll
        for (int kk = 0; kk < NV; ++kk) red[grp][lg + kk * LPR] = G[kk];
        if (lg == 0) redb[grp] = Gb;
        __syncthreads();
        if (grp == 0) {
            for (int g2 = 1; g2 < GPB; ++g2) {
#pragma unroll
                for (int kk = 0; kk < NV; ++kk) G[kk] += red[g2][lg + kk * LPR];
                Gb += redb[g2];
            }
            const float cnt = (float)rec.w;
            const float kc = k.kappa * cnt;
#pragma unroll
            for (int kk = 0; kk < NV; ++kk) G[kk] += kc * Wv[kk];
            Gb += k.kappa_b * cnt * bval;
            fn.finish(is_row, id, wid, code & 0x3fffffff, G, Wv, Gb, bval, st);
        }
        return false;
    }

    // ---- light ids: one group each, dealt round-robin over the light blocks
    const int nu_r = wk.nu_r_host >= 0 ? wk.nu_r_host : wk.counts[1];
    const int nu_c = wk.nu_c_host >= 0 ? wk.nu_c_host : wk.counts[3];
    const int q_begin = (wk.sides & 1) ? 0 : nu_r;
    const int total = (wk.sides & 2) ? nu_r + nu_c : nu_r;
    // the last workgroup of the grid only does the once-per-step scalar work, beside everyone else
    if ((int)blockIdx.x == nblocks - 1) return (wk.sides & 2) != 0;
    const int lb = blockIdx.x - wk.heavy_blocks, nlb = nblocks - wk.heavy_blocks - 1;
    if (wk.flips) {
        // twin form, list drawn by the col-side launch: the row ids one run of the row pass held completely have their new
        // row in the other copy — flip their version now that no gather reads the old one (ids are distinct: a thread per byte;
        // the ids on the list are not among them)
        for (int q = lb * kBlock + (int)threadIdx.x; q < nu_r; q += nlb * kBlock) {
            const int4 rec = reinterpret_cast<const int4 *>(rs.uniq_rec)[q];
            if (rec.z <= wk.heavy_chunks && Slots(rec.y, rec.z, wk.per).count == 1) rs.ver[rec.x] ^= 1;
        }
    }
    // behind a FUSE pass triage_kernel has listed the few ids that still need work: walk that list instead of all ids
    const int n_items = wk.work ? wk.work[0] : total - q_begin;
    for (int it = lb * GPB + grp; it < n_items; it += nlb * GPB) {
        const int q = wk.work ? wk.work[4 + it] : q_begin + it;
        const bool is_row = q < nu_r;
        const SideBufs &sb = is_row ? rs : cs;
        const int qq = is_row ? q : q - nu_r;
        const int4 rec = reinterpret_cast<const int4 *>(sb.uniq_rec)[qq];   // {id, first chunk, chunks, pairs}
        if (rec.z > wk.heavy_chunks) continue;                               // a heavy block has it
        GLOVE_DRAIN(); GLOVE_STAMP(1);      // record arrived
        const int32_t id = rec.x;
        const int pre = is_row ? wk.pre_r : wk.pre_c;
        const Slots sl(rec.y, rec.z, pre != kFuseNone ? wk.per : 1, pre != kFuseNone ? wk.gpb : 0);
        const int sl0 = sl.f;
        if (pre != kFuseNone && sl.one_group) {
            // one run held the whole id and the pass kernel already applied it (sidepass_kernel FUSE): in place ->
            // nothing left to do; into its slot -> move the finished row and bias into the table now that no pass
            // reads the old ones; twin -> the other copy holds the new row: flip the version
            if (pre == kFuseSlot) {
                f4 Wn[NV];
                load_row<LPR, NV>(Wn, sb.gp, sl0, d4, lg);
                const float bn = sb.gb[sl0];
                store_row<LPR, NV>(sb.W, (size_t)id, d4, lg, Wn);
                if (lg == 0) sb.bias[id] = bn;
            }
            if (pre == kFuseTwin && lg == 0) sb.ver[id] ^= 1;
            continue;
        }
        const int32_t wid = cur_row(sb, id);
        const float cnt = (float)rec.w;
        f4 G[NV], Wv[NV];
        typename F::State st;
        load_row<LPR, NV>(G, sb.gp, sl0, d4, lg);
        float Gb = sb.gb[sl0];
        load_row<LPR, NV>(Wv, sb.W, wid, d4, lg);
        const float bval = sb.bias[wid];
        fn.prefetch(is_row, id, st);
        sum_partials<LPR, NV>(sb, sl, 1, 1, d4, lg, G, Gb);
        const float kc = k.kappa * cnt;
#pragma unroll
        for (int kk = 0; kk < NV; ++kk) G[kk] += kc * Wv[kk];
        Gb += k.kappa_b * cnt * bval;
        GLOVE_DRAIN(); GLOVE_STAMP(3);      // rows arrived
        fn.finish(is_row, id, wid, qq, G, Wv, Gb, bval, st);
        GLOVE_DRAIN(); GLOVE_STAMP(4);      // stores retired
    }
    GLOVE_STAMP(5);
    return false;
}

// Deterministic sum of the rowpass block partials by the whole workgroup (thread t takes blocks
// t, t+256, ...; then lanes, then waves, in a fixed order).  Result valid in thread 0.
__device__ inline void sum_blockpart(const float *blockpart, int nblocks, float (&tot)[kPartials])
{
    __shared__ float red2[kBlock / 64][kPartials];
    f4 acc = f4{0.f, 0.f, 0.f, 0.f};
    const f4 *bp = reinterpret_cast<const f4 *>(blockpart);
#pragma unroll
    for (int it = 0; it < kMaxBlocks / kBlock; ++it) {
        const int b = threadIdx.x + it * kBlock;
        const f4 v = bp[b < nblocks ? b : 0];
        acc += (b < nblocks) ? v : f4{0.f, 0.f, 0.f, 0.f};
    }
    // fused passes of big batches only (up to kMaxPassBlocks workgroups): same order, eight loads in flight at a time —
    // one dependent load per round was 12 us of the C4 apply launch
    for (int b0 = threadIdx.x + kMaxBlocks; b0 < nblocks; b0 += 8 * kBlock) {
        f4 v[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            const int b = b0 + x * kBlock;
            v[x] = bp[b < nblocks ? b : 0];
        }
#pragma unroll
        for (int x = 0; x < 8; ++x) acc += (b0 + x * kBlock < nblocks) ? v[x] : f4{0.f, 0.f, 0.f, 0.f};
    }
    tot[0] = wave_sum(acc.x); tot[1] = wave_sum(acc.y); tot[2] = wave_sum(acc.z); tot[3] = wave_sum(acc.w);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < kPartials; ++i) red2[threadIdx.x >> 6][i] = tot[i];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < kPartials; ++i) {
            float sacc = 0.f;
#pragma unroll
            for (int wv = 0; wv < kBlock / 64; ++wv) sacc += red2[wv][i];
            tot[i] = sacc;
        }
    }
}

__device__ inline void loss_from_partials(const float (&tot)[kPartials], const StepConsts &k, float g,
                                          float &loss, float &L, float &reg)
{
    // (no contraction: left to the compiler, the products fused differently in different epilogues — the touched-rows exchange
    // reported Adamax's and Nadam's loss a few bits away from the single-GPU step's on the same partials)
#pragma clang fp contract(off)
    // tot = {sum w diff^2, sum |r|^2+|c|^2, sum br^2+bc^2, sum e}
    L = tot[0] * k.inv_batch;
    reg = k.l2 * k.inv_d * k.inv_batch * tot[1] + k.l2 * k.inv_batch * tot[2] + k.l2 * g * g;
    loss = L + k.m * reg;
}

// The once-per-step scalar work, one thread: from the summed partials `tot` and the global bias with its slots as the step began
// (from[0], from[1], TWO: from[2]) to the loss scalars (loss_out, unless null) and the bias the next step begins with
// (to[0 ..]: update(bias, slot 1, slot 2, dg) is the optimizer at hand on the bias gradient dg).
// CONTRACT_DG = false: dg as a rounded product and a sum of their own (the fused Nadam step has always formed it so)
template <bool TWO, bool CONTRACT_DG = true, class F>
__device__ inline void scalar_epilogue(const float (&tot)[kPartials], const StepConsts &k, const float *from, float *to, F update,
                                       float *loss_out)
{
    float gs[3] = {from[0], from[1], TWO ? from[2] : 0.f};
    const float g = gs[0];
    float loss, L, reg;
    loss_from_partials(tot, k, g, loss, L, reg);
    float dg;
    if (CONTRACT_DG) {
        dg = tot[3] + 2.0f * k.m * k.l2 * g;
    } else {
#pragma clang fp contract(off)
        dg = tot[3] + 2.0f * k.m * k.l2 * g;
    }
    update(gs[0], gs[1], gs[2], dg);
    to[0] = gs[0];
    to[1] = gs[1];
    if (TWO) to[2] = gs[2];
    if (loss_out) { loss_out[0] = loss; loss_out[1] = L; loss_out[2] = reg; loss_out[3] = tot[3]; }
}

// Behind a FUSE pass most ids are finished: the launch that applies the rest spent its time on one dependent record load
// per id, 20 ids per lane group in a row (V = 400 k: 57 us for 24 MB of traffic).  One THREAD per distinct id sorts
// them out first: finished ids of a twinned row table get their version flipped right here, finished ids of the
// in-place side need nothing, and the positions of the light ids that still need work — a copy out of a slot, or the
// sum of several runs — go onto a list (work[0] counts them; the row pass zeroed it).  The list's order varies from
// run to run, the work items are independent: results do not depend on it.  Heavy ids keep their own workgroups.
__global__ __launch_bounds__(kBlock) void triage_kernel(IdWork wk, SideBufs rs, SideBufs cs, int32_t *__restrict__ work)
{
    const int nu_r = wk.nu_r_host >= 0 ? wk.nu_r_host : wk.counts[1];
    const int nu_c = wk.nu_c_host >= 0 ? wk.nu_c_host : wk.counts[3];
    const int q = blockIdx.x * kBlock + threadIdx.x;
    if (q >= nu_r + nu_c) return;
    const bool is_row = q < nu_r;
    if (!(wk.sides & (is_row ? 1 : 2))) return;          // not a side of this step
    const int4 rec = is_row ? reinterpret_cast<const int4 *>(rs.uniq_rec)[q] : reinterpret_cast<const int4 *>(cs.uniq_rec)[q - nu_r];
    if (rec.z > wk.heavy_chunks) return;
    const int pre = is_row ? wk.pre_r : wk.pre_c;
    const bool whole = pre != kFuseNone && Slots(rec.y, rec.z, wk.per).count == 1;
    if (whole && pre == kFuseInPlace) return;
    if (whole && pre == kFuseTwin) {
        rs.ver[rec.x] ^= 1;                 // ids are distinct: one thread per byte
        return;
    }
    work[4 + atomicAdd(work, 1)] = q;
}

// The loss partials of a row pass with `nblocks` workgroups, folded into entry 0 (the rest zeroed): any later reader that
// sums entries 0 .. n-1 for its own idea of n >= 1 (the classic row pass's grid) finds the same totals.
__global__ __launch_bounds__(kBlock) void fold_blockpart_kernel(float *__restrict__ blockpart, int nblocks)
{
    float tot[kPartials];
    sum_blockpart(blockpart, nblocks, tot);
    __shared__ float keep[kPartials];
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < kPartials; ++i) keep[i] = tot[i];
    }
    __syncthreads();                        // everybody has read its share before anything is overwritten
    for (int i = threadIdx.x; i < kMaxPassBlocks * kPartials; i += kBlock) blockpart[i] = i < kPartials ? keep[i] : 0.f;
}

// The loss partials of the last row pass as they travel in a packed list's header: {sum e, sum w diff^2, sum |r|^2+|c|^2, sum b^2}
__global__ __launch_bounds__(kBlock) void loss_partials_kernel(const float *__restrict__ blockpart, int nblocks, float *__restrict__ out)
{
    float tot[kPartials];
    sum_blockpart(blockpart, nblocks, tot);
    if (threadIdx.x == 0) { out[0] = tot[3]; out[1] = tot[0]; out[2] = tot[1]; out[3] = tot[2]; }
}

template <int LPR, int NV>
struct AdagradApply {
    SideBufs rs, cs;
    int d4, lg;
    float lr, eps;
    struct State { f4 A[NV]; float Ab; };
    __device__ void prefetch(bool is_row, int32_t id, State &st) const
    {
        const SideBufs &sb = is_row ? rs : cs;
        load_row<LPR, NV>(st.A, sb.S1, id, d4, lg);
        st.Ab = sb.S1b[id];
    }
    __device__ void finish(bool is_row, int32_t id, int32_t wid, int q, f4 (&G)[NV], f4 (&Wv)[NV], float Gb, float bval, State &st) const
    {
        const SideBufs &sb = is_row ? rs : cs;
#pragma unroll
        for (int kk = 0; kk < NV; ++kk) adagrad_vec(Wv[kk], st.A[kk], G[kk], lr, eps);
        store_row<LPR, NV>(sb.S1, (size_t)id, d4, lg, st.A);
        store_row<LPR, NV>(sb.W, (size_t)wid, d4, lg, Wv);
        if (lg == 0) {
            adagrad_elem(bval, st.Ab, Gb, lr, eps);
            sb.S1b[id] = st.Ab;
            sb.bias[wid] = bval;
        }
    }
};

template <int LPR, int NV>
__global__ __launch_bounds__(kBlock) void apply_adagrad_kernel(
    IdWork wk, SideBufs rs, SideBufs cs, int d4, StepConsts k,
    float *__restrict__ scalars, const float *__restrict__ blockpart, int nblocks_rowpass,
    float *__restrict__ loss_out)
{
    const bool scalar_duty = for_each_id<LPR, NV>(wk, rs, cs, d4, k,
                                                  AdagradApply<LPR, NV>{rs, cs, d4, (int)(threadIdx.x % LPR), k.lr, k.eps});
    // global bias (dense Adagrad) + loss scalars: one (light) workgroup
    if (scalar_duty) {
        float tot[kPartials];
        sum_blockpart(blockpart, nblocks_rowpass, tot);
        if (threadIdx.x == 0)
            scalar_epilogue<false>(tot, k, scalars, scalars, [&](float &gn, float &Ag, float &, float dg) { adagrad_elem(gn, Ag, dg, k.lr, k.eps); },
                                   loss_out);
    }
    GLOVE_DRAIN(); GLOVE_STAMP(6);
}

// Adds this plan's summed gradients into the dense buffers (no two work items share an id
// within one side, so plain read-modify-write is race free).
template <int LPR, int NV>
struct DenseGradAdd {
    float *G_R, *G_C, *G_br, *G_bc;
    int d4, lg;
    struct State { f4 old[NV]; float oldb; };
    __device__ void prefetch(bool is_row, int32_t id, State &st) const
    {
        load_row<LPR, NV>(st.old, is_row ? G_R : G_C, id, d4, lg);
        st.oldb = (is_row ? G_br : G_bc)[id];
    }
    __device__ void finish(bool is_row, int32_t id, int32_t wid, int q, f4 (&G)[NV], f4 (&Wv)[NV], float Gb, float bval, State &st) const
    {
        (void)Wv; (void)bval;
#pragma unroll
        for (int kk = 0; kk < NV; ++kk) st.old[kk] += G[kk];
        store_row<LPR, NV>(is_row ? G_R : G_C, (size_t)id, d4, lg, st.old);
        if (lg == 0) (is_row ? G_br : G_bc)[id] = st.oldb + Gb;
    }
};

template <int LPR, int NV>
__global__ __launch_bounds__(kBlock) void dense_grad_kernel(
    IdWork wk, SideBufs rs, SideBufs cs, int d4, StepConsts k,
    float *__restrict__ G_R, float *__restrict__ G_C, float *__restrict__ G_br, float *__restrict__ G_bc,
    float *__restrict__ tail, const float *__restrict__ blockpart, int nblocks_rowpass)
{
    const bool scalar_duty = for_each_id<LPR, NV>(wk, rs, cs, d4, k,
                                                  DenseGradAdd<LPR, NV>{G_R, G_C, G_br, G_bc, d4, (int)(threadIdx.x % LPR)});
    if (scalar_duty) {
        float tot[kPartials];
        sum_blockpart(blockpart, nblocks_rowpass, tot);
        if (threadIdx.x == 0) {
            tail[0] += tot[3];   // sum e
            tail[1] += tot[0];   // sum w diff^2
            tail[2] += tot[1];   // sum |r|^2 + |c|^2
            tail[3] += tot[2];   // sum br^2 + bc^2
        }
    }
}

// ------------------------------------------------------------------------------------------
// Touched-rows exchange: instead of a dense [V,d] gradient buffer a rank hands over ONE packed list
// of (id, summed gradient row) per step.  An entry is d + 4 floats, 16-B aligned:
//     [ gradient row, d floats | bias gradient | id (int bits) | side (0 row, 1 col; int bits) | 0 ]
// Entry 0 of a list is its header: [row entries, col entries (int bits) | sum e, sum w diff^2, sum |r|^2+|c|^2,
// sum br^2+bc^2 | 0 ...]; the row-side entries follow in plan order (ascending id), then the col-side entries.
// The receiving side adds the lists of all ranks into the dense buffer G_flat IN LIST ORDER (one launch per list: ids are
// distinct within a list, launches are ordered, so the sum over ranks has a fixed order), the first list that touches an id
// storing instead of adding (G_flat needs no zeroing) and leaving its tag in `mark`; then one launch applies Adagrad to
// every touched id, each from the list that touched it first, and clears the marks.
// ------------------------------------------------------------------------------------------
constexpr int kPackExtra = 4;

template <int LPR, int NV>
struct PackGrad {
    float *packed;
    int d4, lg, row_entries;
    struct State {};
    __device__ void prefetch(bool, int32_t, State &) const {}
    __device__ void finish(bool is_row, int32_t id, int32_t wid, int q, f4 (&G)[NV], f4 (&Wv)[NV], float Gb, float bval, State &) const
    {
        (void)Wv; (void)bval;
        const size_t stride4 = (size_t)d4 + 1;
        f4 *e = reinterpret_cast<f4 *>(packed) + (size_t)(1 + (is_row ? q : row_entries + q)) * stride4;
#pragma unroll
        for (int kk = 0; kk < NV; ++kk) {
            const int i4 = lg + kk * LPR;
            if (i4 < d4) e[i4] = G[kk];
        }
        if (lg == 0) e[d4] = f4{Gb, __int_as_float(id), __int_as_float(is_row ? 0 : 1), 0.f};
    }
};

template <int LPR, int NV>
__global__ __launch_bounds__(kBlock) void pack_grad_kernel(
    IdWork wk, SideBufs rs, SideBufs cs, int d4, StepConsts k, float *__restrict__ packed,
    const float *__restrict__ blockpart, int nblocks_rowpass)
{
    const int nu_r = wk.nu_r_host >= 0 ? wk.nu_r_host : wk.counts[1];
    const int nu_c = wk.nu_c_host >= 0 ? wk.nu_c_host : wk.counts[3];
    const int row_entries = (wk.sides & 1) ? nu_r : 0;
    const bool scalar_duty = for_each_id<LPR, NV>(wk, rs, cs, d4, k,
                                                  PackGrad<LPR, NV>{packed, d4, (int)(threadIdx.x % LPR), row_entries});
    if (scalar_duty) {                      // the col side carries the loss partials (glove_hyper.sides)
        float tot[kPartials];
        sum_blockpart(blockpart, nblocks_rowpass, tot);
        if (threadIdx.x == 0) {
            f4 *h = reinterpret_cast<f4 *>(packed);
            h[0] = f4{__int_as_float(row_entries), __int_as_float(nu_c), tot[3], tot[0]};
            h[1] = f4{tot[1], tot[2], 0.f, 0.f};
        }
    } else if (!(wk.sides & 2) && blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        f4 *h = reinterpret_cast<f4 *>(packed);            // row side only: no loss partials travel with it
        h[0] = f4{__int_as_float(row_entries), __int_as_float(0), 0.f, 0.f};
        h[1] = f4{0.f, 0.f, 0.f, 0.f};
    }
}

struct PackedList {
    const float *entries;       // first entry behind the header (or a bare array of entries)
    const int32_t *ids;         // if not null: ids[i] replaces the id stored in entry i (owner-local indices)
    const float *header;        // if not null: entry count = row entries + col entries of this header
    int n_host;                 // else the entry count
    int side;                   // -1: every entry names its side; 0 / 1: all entries are of that side
};

struct DenseViews { float *G_R, *G_br, *G_C, *G_bc; int32_t *mark; int V_row; };

__device__ inline int packed_count(const PackedList &pl)
{
    if (!pl.header) return pl.n_host;
    return __float_as_int(pl.header[0]) + __float_as_int(pl.header[1]);
}

// mark[id]: bits 0..7 = how many lists touch the id (count_packed_kernel; 0 = not counted), bits 8.. = 1 + tag of the
// first list that stored the id's row in the dense buffer (0 = none yet)
constexpr int kMarkCountBits = 8, kMarkCountMask = (1 << kMarkCountBits) - 1;

// (count_packed_kernel below is the optional first pass over ALL lists: afterwards an id only one list touches needs no
// trip through the dense buffer — the apply kernel takes its gradient straight from that list's entry, combine skips it.)

template <int LPR, int NV>
__global__ __launch_bounds__(kBlock) void combine_packed_kernel(PackedList pl, int tag, DenseViews dv, int d4)
{
    constexpr int GPB = kBlock / LPR;
    const int lg = threadIdx.x % LPR, grp = threadIdx.x / LPR;
    const int n = packed_count(pl);
    const size_t stride4 = (size_t)d4 + 1;
    for (int i = blockIdx.x * GPB + grp; i < n; i += gridDim.x * GPB) {
        const f4 *e = reinterpret_cast<const f4 *>(pl.entries) + (size_t)i * stride4;
        const f4 x = e[d4];
        const int32_t id = pl.ids ? pl.ids[i] : __float_as_int(x.y);
        const bool is_row = (pl.side >= 0 ? pl.side : __float_as_int(x.z)) == 0;
        int32_t *mk = dv.mark + (is_row ? 0 : dv.V_row) + id;
        const int32_t m = *mk;              // every lane of the group reads it before lane 0 rewrites it below
        if ((m & kMarkCountMask) == 1) continue;        // counted, and this list alone touches the id: applied from the entry
        const int32_t seen = m >> kMarkCountBits;
        f4 g[NV];
#pragma unroll
        for (int kk = 0; kk < NV; ++kk) {
            const int i4 = lg + kk * LPR;
            g[kk] = e[i4 < d4 ? i4 : d4 - 1];
        }
        float *Gt = is_row ? dv.G_R : dv.G_C;
        float *Gb = is_row ? dv.G_br : dv.G_bc;
        if (seen != 0) {                    // a list before this one touched the id: add behind it
            f4 old[NV];
            load_row<LPR, NV>(old, Gt, id, d4, lg);
#pragma unroll
            for (int kk = 0; kk < NV; ++kk) g[kk] = old[kk] + g[kk];
        }
        store_row<LPR, NV>(Gt, (size_t)id, d4, lg, g);
        if (lg == 0) {
            Gb[id] = seen != 0 ? Gb[id] + x.x : x.x;
            if (seen == 0) *mk = m | ((tag + 1) << kMarkCountBits);
        }
    }
}

struct PackedLists { PackedList l[8]; int n; };

__global__ __launch_bounds__(kBlock) void count_packed_kernel(PackedLists pls, DenseViews dv, int d4)
{
    const PackedList &pl = pls.l[blockIdx.y];
    const int n = packed_count(pl);
    const size_t stride = ((size_t)d4 + 1) * 4;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const float *x = pl.entries + (size_t)i * stride + (size_t)d4 * 4;
        const int32_t id = pl.ids ? pl.ids[i] : __float_as_int(x[1]);
        const bool is_row = (pl.side >= 0 ? pl.side : __float_as_int(x[2])) == 0;
        atomicAdd(dv.mark + (is_row ? 0 : dv.V_row) + id, 1);
    }
}

// More than eight lists and no summed tail from the caller: the loss partials of ALL headers are added up first, eight
// lists per launch in list order, into four scratch floats (the reserved half of G_flat's tail).
__global__ void sum_headers_kernel(PackedLists pls, float *__restrict__ acc4, int first)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    float t[4] = {0.f, 0.f, 0.f, 0.f};
    if (!first) { t[0] = acc4[0]; t[1] = acc4[1]; t[2] = acc4[2]; t[3] = acc4[3]; }
    for (int r = 0; r < pls.n; ++r) {
        const float *h = pls.l[r].header;
        if (h) { t[0] += h[2]; t[1] += h[3]; t[2] += h[4]; t[3] += h[5]; }
    }
    acc4[0] = t[0]; acc4[1] = t[1]; acc4[2] = t[2]; acc4[3] = t[3];
}

// Keras-legacy Nadam on the same two-part kernel (the legacy optimizer's sparse path decays m and v over the whole variable like
// its Adam, but only the touched rows move: optimizer_v2/nadam.py `_resource_apply_sparse`; restated in oracle/glove_ref.py _nadam).
// The momentum cache — the running product of the schedule u_i = beta1 (1 - 0.5 0.96^(0.004 i)) — lives in scalars[4 + parity]:
// step t reads slot (t - 1) & 1 and its scalar epilogue writes slot t & 1, so no workgroup of step t sees the new value.
struct NadamConsts { float lr, eps, b1, b2, one_minus_u_t, u_t1, om_new, om_next, v_den, sched_new; };
__device__ inline NadamConsts nadam_consts(float lr, float eps, float b1, float b2, double ln_beta2, int64_t t, const float *scalars)
{
#pragma clang fp contract(off)
    const double ln096 = -0.040821994520255166;                 // ln 0.96
    const float u_t = b1 * (1.0f - 0.5f * expf((float)(0.004 * (double)t * ln096)));
    const float u_t1 = b1 * (1.0f - 0.5f * expf((float)(0.004 * (double)(t + 1) * ln096)));
    const float cache = scalars[4 + (int)((t - 1) & 1)];
    NadamConsts k;
    k.lr = lr; k.eps = eps; k.b1 = b1; k.b2 = b2;
    k.sched_new = cache * u_t;
    k.one_minus_u_t = 1.0f - u_t;
    k.u_t1 = u_t1;
    k.om_new = 1.0f - k.sched_new;
    k.om_next = 1.0f - k.sched_new * u_t1;
    k.v_den = -expm1f((float)((double)t * ln_beta2));
    return k;
}
__device__ inline void nadam_elem(float &w, float &m, float &v, float g, const NadamConsts &k)
{
#pragma clang fp contract(off)
    m = m * k.b1 + (1.0f - k.b1) * g;
    v = v * k.b2 + (1.0f - k.b2) * g * g;
    const float m_bar = k.one_minus_u_t * (g / k.om_new) + k.u_t1 * (m / k.om_next);
    w -= k.lr * m_bar / (sqrtf(v / k.v_den) + k.eps);
}

// ---- the element updates of the per-row optimizers (SGD, Adamax, Adadelta, Ftrl, LazyAdam, RowWiseAdagrad): include/glove_hip.h
// glove_hyper.optimizer; used by the apply epilogues of the single-GPU step (SparseOptApply) and of the touched-rows exchange
// (apply_packed_kernel)
struct OptConsts { float lr, eps, momentum, lr_t, b1, b2; int nesterov; float rho; };
template <int OPT> struct OptSlots {
    static constexpr bool two = OPT == GLOVE_OPT_ADAMAX || OPT == GLOVE_OPT_ADADELTA || OPT == GLOVE_OPT_FTRL || OPT == GLOVE_OPT_NADAM ||
                                OPT == GLOVE_OPT_ADAM || OPT == GLOVE_OPT_LAZYADAM;
    // RowWiseAdagrad: slot 1 of an embedding table is ONE float per row (float[rows], indexed by id, not by id * d)
    static constexpr bool row_wise = OPT == GLOVE_OPT_ROWWISE_ADAGRAD;
};

// RowWiseAdagrad on one embedding row, held by its group of LPR lanes (every lane of the group is here): G is the id's COMPLETE
// summed gradient (activity-L2 term in; the lanes and columns past the row end hold 0 and add nothing), A the row's one
// accumulator, the same in every lane on entry and on return.  A += (sum_j G_j^2) / d_model, then W -= lr G / (sqrt(A) + eps)
// with the incremented A.  The sum has a fixed order (dot4 chains per lane, then the group butterfly) and the rounding sequence
// is spelled out: both kernels that apply it give the same bits.
template <int LPR, int NV>
__device__ inline void rowwise_adagrad_row(f4 (&Wv)[NV], float &A, const f4 (&G)[NV], float lr, float eps, float inv_d)
{
#pragma clang fp contract(off)
    float sq = 0.f;
#pragma unroll
    for (int kk = 0; kk < NV; ++kk) sq += dot4(G[kk], G[kk]);
    sq = group_sum<LPR>(sq);
    A += sq * inv_d;
    const float scale = lr * inv_sqrt_eps(A, eps);
#pragma unroll
    for (int kk = 0; kk < NV; ++kk) Wv[kk] -= scale * G[kk];
}
template <int OPT>
struct OptElem {
    // Adadelta (kernel SparseApplyAdadelta): a = accum_grad, u = accum_var
    __device__ static void adadelta(float &w, float &a, float &u, float g, const OptConsts &o)
    {
#pragma clang fp contract(off)
        a = a * o.rho + g * g * (1.0f - o.rho);
        const float upd = sqrtf(u + o.eps) / sqrtf(a + o.eps) * g;
        w -= upd * o.lr;
        u = u * o.rho + upd * upd * (1.0f - o.rho);
    }
    // Ftrl at its Keras defaults (kernel FtrlCompute; lr_power -0.5, l1 = l2 = 0): a = accumulator, z = linear
    __device__ static void ftrl(float &w, float &a, float &z, float g, const OptConsts &o)
    {
#pragma clang fp contract(off)
        const float na = a + g * g;
        z += g - (sqrtf(na) - sqrtf(a)) / o.lr * w;
        w = fabsf(z) > 0.f ? -z / (sqrtf(na) / o.lr) : 0.f;
        a = na;
    }
    __device__ static void sgd(float &w, float &a, float g, const OptConsts &o)
    {
#pragma clang fp contract(off)
        if (o.momentum == 0.f) { w -= o.lr * g; return; }
        a = a * o.momentum - o.lr * g;
        w += o.nesterov ? a * o.momentum - o.lr * g : a;
    }
    __device__ static void adamax(float &w, float &m, float &v, float g, const OptConsts &o)
    {
#pragma clang fp contract(off)
        m = o.b1 * m + (1.0f - o.b1) * g;
        v = fmaxf(o.b2 * v, fabsf(g));
        w -= o.lr_t * m / (v + o.eps);
    }
    // RowWiseAdagrad's per-row floats (br, bc, the global bias): Keras Adagrad as adagrad_elem, the rounding sequence spelled out so
    // that the single-GPU apply and the packed apply give the same bits
    __device__ static void adagrad(float &w, float &a, float g, const OptConsts &o)
    {
#pragma clang fp contract(off)
        a += g * g;
        w -= o.lr * g * inv_sqrt_eps(a, o.eps);
    }
    // RMSprop as dense_rmsprop_kernel spells it (a = rms): the entry's rms takes (1 - rho) g^2, the weight moves where g != 0
    __device__ static void rmsprop(float &w, float &a, float g, const OptConsts &o)
    {
#pragma clang fp contract(off)
        a = o.rho * a + (1.0f - o.rho) * g * g;
        if (g != 0.f) w -= o.lr * g / (sqrtf(a) + o.eps);
    }
    // (nk: Nadam's constants of this step — the touched-rows exchange only: apply_packed_kernel; a = m, b = v.  Adam: a = m,
    // b = v, o.lr_t of this step — the touched-rows exchange only, the rows no list names take the sweep's G = 0 update.
    // LazyAdam: Adam's element update on the touched rows alone, no sweep anywhere: every other row keeps its bits.
    // RowWiseAdagrad: the variables that are one float per row anyway — br, bc, the global bias — take plain Adagrad; the
    // embedding rows never come here: rowwise_adagrad_row)
    __device__ static void one(float &w, float &a, float &b, float g, const OptConsts &o, const NadamConsts &nk)
    {
        if (OPT == GLOVE_OPT_ROWWISE_ADAGRAD) adagrad(w, a, g, o);
        else if (OPT == GLOVE_OPT_SGD) sgd(w, a, g, o);
        else if (OPT == GLOVE_OPT_ADAMAX) adamax(w, a, b, g, o);
        else if (OPT == GLOVE_OPT_ADADELTA) adadelta(w, a, b, g, o);
        else if (OPT == GLOVE_OPT_NADAM) nadam_elem(w, a, b, g, nk);
        else if (OPT == GLOVE_OPT_RMSPROP) rmsprop(w, a, g, o);
        else if (OPT == GLOVE_OPT_ADAM || OPT == GLOVE_OPT_LAZYADAM) adam_elem(w, a, b, g, o.lr_t, o.b1, o.b2, o.eps);
        else ftrl(w, a, b, g, o);
    }
    __device__ static void one(float &w, float &a, float &b, float g, const OptConsts &o) { one(w, a, b, g, o, NadamConsts{}); }
};

// A lane group walks entries gg, gg + TG, gg + 2 TG, ... (TG lane groups in the launch).  Looked up one entry at a time
// that is three dependent round trips per entry (id -> mark -> rows) and ~16 entries per group at C5, a latency chain.
// Instead the group's LPR lanes look LPR entries up at once — lane t the id, side, bias gradient and mark of the t-th
// of them — and the rows are then moved two entries at a time, what each needs handed round by lane shuffles: one
// round trip per pair of entries.
// OPT: GLOVE_OPT_ADAGRAD, or one of the per-row optimizers (OptElem: SGD, Adamax, Adadelta, Ftrl, LazyAdam, RowWiseAdagrad) — only touched rows move
// under all of them, so the exchange is the same and the epilogue differs.  The dense-decay ones (Nadam, Adam, RMSprop) move
// every row's slots every step: decay_unmarked_kernel gives the rows no list names their G = 0 update first, and the listed
// rows take the epilogue here.  s2: the second slot of every variable where the optimizer has one (scalars[2] for the global bias).
struct SlotTwo { float *R, *C, *br, *bc; };

constexpr int kSweepRows = 2;       // table rows a sweep lane group keeps in flight (adam_fused_kernel, decay_unmarked_kernel)

// ---- the sweep of the dense-decay optimizers: every row of [lo, hi) of the concatenation [row side | col side] that the step's
// other workgroups (or its next launch) do not own takes the G = 0 update
//   Nadam    m and v decay (Keras' legacy sparse Nadam decays them over the whole variable; the row stays)
//   Adam     m and v decay and the row moves: W -= lr_t m / (sqrt(v) + eps)
//   RMSprop  the rms slot decays (rho rms + (1 - rho) 0 = rho rms: dense_rmsprop_kernel's bits on a zero gradient)
// A pure stream: a lane group per row, kSweepRows rows in flight per group, everything requested before the mark is looked at
// (what an owned row loaded is dropped).  Lane group `first` of `stride` takes rows first, first + stride, ...
// The kind of mark that says who owns a row:
struct FloatMarks {                 // the fused step: the passes left 1.0f for every id of the batch (in the bias segments of G_flat,
    float *rows, *cols;             // otherwise unused on this path); the sweep clears it — G_flat is all zero again afterwards
    typedef float Raw;
    __device__ Raw load(bool live, bool is_row, int id, int) const { return live ? (is_row ? rows : cols)[id] : 1.0f; }
    __device__ static bool owned(Raw m) { return m != 0.f; }
    __device__ void clear(bool is_row, int id) const { (is_row ? rows : cols)[id] = 0.f; }
};
struct CountMarks {                 // the touched-rows exchange: count bits in the mark of every id some list names
    const int32_t *mark;            // (count_packed_kernel); they stay for apply_packed_kernel, the next launch
    typedef int Raw;
    __device__ Raw load(bool live, bool, int, int v) const { return live ? mark[v] & kMarkCountMask : 1; }
    __device__ static bool owned(Raw m) { return m != 0; }
    __device__ void clear(bool, int) const {}
};

template <int LPR, int NV, int OPT, class MARKS>
__device__ inline void sweep_unowned(const MARKS &marks, const SideBufs &rs, const SideBufs &cs, const SlotTwo &s2, int V_row, int d4,
                                     int first, int stride, int hi, float lr_t, float b1, float b2, float rho, float eps)
{
    constexpr bool kW = OPT == GLOVE_OPT_ADAM;                  // the row itself moves
    constexpr bool kTwo = OPT != GLOVE_OPT_RMSPROP;             // m and v; RMSprop has its rms only
    const int lg = threadIdx.x % LPR;
    for (int v0 = first; v0 < hi; v0 += kSweepRows * stride) {
        f4 Wv[kSweepRows][kW ? NV : 1], M[kSweepRows][NV], Vv[kSweepRows][kTwo ? NV : 1];
        typename MARKS::Raw mk[kSweepRows];
        float bval[kSweepRows], Mb[kSweepRows], Vb[kSweepRows];
#pragma unroll
        for (int r = 0; r < kSweepRows; ++r) {
            const int v = v0 + r * stride;
            const bool live = v < hi;
            const bool is_row = v < V_row;
            const int id = live ? (is_row ? v : v - V_row) : 0;
            const SideBufs &sb = is_row ? rs : cs;
            mk[r] = marks.load(live, is_row, id, v);
            if constexpr (kW) load_row<LPR, NV>(Wv[r], sb.W, id, d4, lg);
            load_row<LPR, NV>(M[r], sb.S1, id, d4, lg);
            if constexpr (kTwo) load_row<LPR, NV>(Vv[r], is_row ? s2.R : s2.C, id, d4, lg);
            bval[r] = Mb[r] = Vb[r] = 0.f;
            if (lg == 0) {
                if constexpr (kW) bval[r] = sb.bias[id];
                Mb[r] = sb.S1b[id];
                if constexpr (kTwo) Vb[r] = (is_row ? s2.br : s2.bc)[id];
            }
        }
#pragma unroll
        for (int r = 0; r < kSweepRows; ++r) {
            const int v = v0 + r * stride;
            if (v >= hi) continue;
            const bool is_row = v < V_row;
            const int id = is_row ? v : v - V_row;
            const SideBufs &sb = is_row ? rs : cs;
            if (MARKS::owned(mk[r])) {                           // not this sweep's row
                if (lg == 0) marks.clear(is_row, id);
                continue;
            }
            if constexpr (OPT == GLOVE_OPT_ADAM) {
                const f4 zero = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kk = 0; kk < NV; ++kk) adam_vec(Wv[r][kk], M[r][kk], Vv[r][kk], zero, lr_t, b1, b2, eps);
                if (lg == 0) adam_elem(bval[r], Mb[r], Vb[r], 0.f, lr_t, b1, b2, eps);
            } else if constexpr (OPT == GLOVE_OPT_NADAM) {
#pragma unroll
                for (int kk = 0; kk < NV; ++kk) { M[r][kk] = b1 * M[r][kk]; Vv[r][kk] = b2 * Vv[r][kk]; }
                Mb[r] = b1 * Mb[r];
                Vb[r] = b2 * Vb[r];
            } else {
#pragma unroll
                for (int kk = 0; kk < NV; ++kk) M[r][kk] = rho * M[r][kk];
                Mb[r] = rho * Mb[r];
            }
            store_row<LPR, NV>(sb.S1, (size_t)id, d4, lg, M[r]);
            if constexpr (kTwo) store_row<LPR, NV>(is_row ? s2.R : s2.C, (size_t)id, d4, lg, Vv[r]);
            if constexpr (kW) store_row<LPR, NV>(sb.W, (size_t)id, d4, lg, Wv[r]);
            if (lg == 0) {
                sb.S1b[id] = Mb[r];
                if constexpr (kTwo) (is_row ? s2.br : s2.bc)[id] = Vb[r];
                if constexpr (kW) sb.bias[id] = bval[r];
            }
        }
    }
}

// The dense-decay optimizers on the touched-rows exchange: every row NO rank touched takes the G = 0 update; the rows some rank
// touched are apply_packed_kernel's, the next launch.  Rows [lo, hi) are swept (the sides glove_hyper.sweep_sides selects).
template <int LPR, int NV, int OPT>
__global__ __launch_bounds__(kBlock) void decay_unmarked_kernel(DenseViews dv, SideBufs rs, SideBufs cs, SlotTwo s2, int d4,
                                                                float b1, float b2, float rho, float lr, float eps, double ln_beta1,
                                                                double ln_beta2, const int64_t *__restrict__ step, int lo, int hi)
{
    constexpr int GPB = kBlock / LPR;
    const float lr_t = OPT == GLOVE_OPT_ADAM ? adam_lr_t(lr, ln_beta1, ln_beta2, *step) : 0.f;
    sweep_unowned<LPR, NV, OPT>(CountMarks{dv.mark}, rs, cs, s2, dv.V_row, d4, lo + blockIdx.x * GPB + (int)threadIdx.x / LPR,
                                gridDim.x * GPB, hi, lr_t, b1, b2, rho, eps);
}

template <int LPR, int NV, int OPT>
__global__ __launch_bounds__(kBlock) void apply_packed_kernel(
    PackedLists pls, DenseViews dv, SideBufs rs, SideBufs cs, SlotTwo s2, int d4, StepConsts k, OptConsts o, double ln_beta1,
    double ln_beta2, const int64_t *__restrict__ step, int first_tag, const float *__restrict__ tail_in, float *__restrict__ scalars,
    float *__restrict__ loss_out, int do_scalars)
{
    constexpr int GPB = kBlock / LPR;
    constexpr bool kAdagrad = OPT == GLOVE_OPT_ADAGRAD;
    constexpr bool kTwo = !kAdagrad && OptSlots<OPT>::two;
    constexpr bool kRowWise = OptSlots<OPT>::row_wise;          // slot 1 of R / C: one float per row, no slot row to move
    const bool slots = kAdagrad || !(OPT == GLOVE_OPT_SGD && o.momentum == 0.f);     // (plain SGD keeps no slot)
    // t = global_step as the passes of this step left it (Adamax: lr_t = lr / (1 - beta1^t), as apply_sparse_opt_kernel)
    if (OPT == GLOVE_OPT_ADAMAX) o.lr_t = o.lr / -expm1f((float)((double)(*step) * ln_beta1));
    // Adam (every row moves: the rows no list names took the G = 0 update in decay_unmarked_kernel, the launch before): lr_t of step t
    // (LazyAdam: the same lr_t of the global step, on the listed rows alone — no launch before this one)
    if (OPT == GLOVE_OPT_ADAM || OPT == GLOVE_OPT_LAZYADAM) o.lr_t = adam_lr_t(o.lr, ln_beta1, ln_beta2, *step);
    // Nadam (the ranks' touched rows move; every other row's m and v have decayed in decay_unmarked_kernel, the launch before):
    // the constants of step t = global_step as the passes left it
    NadamConsts nk = {};
    if (OPT == GLOVE_OPT_NADAM) nk = nadam_consts(o.lr, o.eps, o.b1, o.b2, ln_beta2, *step, scalars);
    const int lg = threadIdx.x % LPR, grp = threadIdx.x / LPR;
    const size_t stride4 = (size_t)d4 + 1;
    const PackedList &pl = pls.l[blockIdx.y];
    const int tag = first_tag + blockIdx.y;
    const long n = packed_count(pl);
    const long TG = (long)gridDim.x * GPB, gg = (long)blockIdx.x * GPB + grp;
    const f4 *entries = reinterpret_cast<const f4 *>(pl.entries);
    for (long t0 = 0; gg + t0 * TG < n; t0 += LPR) {
        const long il = gg + (t0 + lg) * TG;
        int32_t id_l = 0;
        int row_l = 1, todo_l = 0;      // todo: 0 nothing (past the end, or another list stored the id first: its entry
        float gb_l = 0.f;               // applies it), 1 this entry is the id's only one: its row IS the sum, 2 the dense buffer has the sum
        if (il < n) {
            const f4 x = entries[il * stride4 + d4];
            id_l = pl.ids ? pl.ids[il] : __float_as_int(x.y);
            row_l = (pl.side >= 0 ? pl.side : __float_as_int(x.z)) == 0;
            gb_l = x.x;
            const int32_t m = dv.mark[(row_l ? 0 : dv.V_row) + id_l];
            todo_l = (m & kMarkCountMask) == 1 ? 1 : ((m >> kMarkCountBits) == tag + 1 ? 2 : 0);
        }
        for (int tt = 0; tt < LPR; tt += 2) {
            if (gg + (t0 + tt) * TG >= n) break;
            int todo[2];
            int32_t id[2];
            bool is_row[2];
            float Gb[2], bval[2], Ab[2], Bb[2], Ar[2];
            f4 G[2][NV], Wv[2][NV], A[2][kRowWise ? 1 : NV], Bv[2][kTwo ? NV : 1];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                todo[e] = __shfl(todo_l, tt + e, LPR);
                id[e] = __shfl(id_l, tt + e, LPR);
                is_row[e] = __shfl(row_l, tt + e, LPR) != 0;
                Gb[e] = __shfl(gb_l, tt + e, LPR);
                Ab[e] = Bb[e] = Ar[e] = 0.f;
            }
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                if (!todo[e]) continue;
                const float *W = is_row[e] ? rs.W : cs.W, *S1 = is_row[e] ? rs.S1 : cs.S1;
                if (todo[e] == 1) {
                    const f4 *row = entries + (size_t)(gg + (t0 + tt + e) * TG) * stride4;
#pragma unroll
                    for (int kk = 0; kk < NV; ++kk) {
                        const int i4 = lg + kk * LPR;
                        const f4 v = row[i4 < d4 ? i4 : d4 - 1];
                        G[e][kk] = (i4 < d4) ? v : f4{0.f, 0.f, 0.f, 0.f};
                    }
                } else {
                    load_row<LPR, NV>(G[e], is_row[e] ? dv.G_R : dv.G_C, id[e], d4, lg);
                    Gb[e] = (is_row[e] ? dv.G_br : dv.G_bc)[id[e]];
                }
                load_row<LPR, NV>(Wv[e], W, id[e], d4, lg);
                bval[e] = (is_row[e] ? rs.bias : cs.bias)[id[e]];
                if (slots) {
                    if constexpr (kRowWise) Ar[e] = S1[id[e]];                      // one float per id, every lane of the group
                    else load_row<LPR, NV>(A[e], S1, id[e], d4, lg);
                    Ab[e] = (is_row[e] ? rs.S1b : cs.S1b)[id[e]];
                }
                if constexpr (kTwo) {
                    load_row<LPR, NV>(Bv[e], is_row[e] ? s2.R : s2.C, id[e], d4, lg);
                    Bb[e] = (is_row[e] ? s2.br : s2.bc)[id[e]];
                }
            }
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                if (!todo[e]) continue;
                float *W = is_row[e] ? rs.W : cs.W, *S1 = is_row[e] ? rs.S1 : cs.S1;
                if constexpr (kAdagrad) {
#pragma unroll
                    for (int kk = 0; kk < NV; ++kk) adagrad_vec(Wv[e][kk], A[e][kk], G[e][kk], k.lr, k.eps);
                } else if constexpr (kRowWise) {
                    // (the whole group holds entry e and then entry e + 1, one after the other: the group's sum is this entry's alone)
                    rowwise_adagrad_row<LPR, NV>(Wv[e], Ar[e], G[e], k.lr, k.eps, k.inv_d);
                } else {
#pragma unroll
                    for (int kk = 0; kk < NV; ++kk) {
                        float w[4] = {Wv[e][kk].x, Wv[e][kk].y, Wv[e][kk].z, Wv[e][kk].w};
                        float a[4] = {A[e][kk].x, A[e][kk].y, A[e][kk].z, A[e][kk].w};
                        float bb[4] = {0.f, 0.f, 0.f, 0.f};
                        if constexpr (kTwo) { bb[0] = Bv[e][kk].x; bb[1] = Bv[e][kk].y; bb[2] = Bv[e][kk].z; bb[3] = Bv[e][kk].w; }
                        const float g[4] = {G[e][kk].x, G[e][kk].y, G[e][kk].z, G[e][kk].w};
#pragma unroll
                        for (int i = 0; i < 4; ++i) OptElem<OPT>::one(w[i], a[i], bb[i], g[i], o, nk);
                        Wv[e][kk] = f4{w[0], w[1], w[2], w[3]};
                        A[e][kk] = f4{a[0], a[1], a[2], a[3]};
                        if constexpr (kTwo) Bv[e][kk] = f4{bb[0], bb[1], bb[2], bb[3]};
                    }
                }
                if constexpr (!kRowWise) {
                    if (slots) store_row<LPR, NV>(S1, (size_t)id[e], d4, lg, A[e]);
                }
                if constexpr (kTwo) store_row<LPR, NV>(is_row[e] ? s2.R : s2.C, (size_t)id[e], d4, lg, Bv[e]);
                store_row<LPR, NV>(W, (size_t)id[e], d4, lg, Wv[e]);
                if (lg == 0) {
                    if constexpr (kRowWise) S1[id[e]] = Ar[e];
                    if constexpr (kAdagrad) adagrad_elem(bval[e], Ab[e], Gb[e], k.lr, k.eps);
                    else OptElem<OPT>::one(bval[e], Ab[e], Bb[e], Gb[e], o, nk);
                    if (slots) (is_row[e] ? rs.S1b : cs.S1b)[id[e]] = Ab[e];
                    if constexpr (kTwo) (is_row[e] ? s2.br : s2.bc)[id[e]] = Bb[e];
                    (is_row[e] ? rs.bias : cs.bias)[id[e]] = bval[e];
                    dv.mark[(is_row[e] ? 0 : dv.V_row) + id[e]] = 0;
                }
            }
        }
    }
    if (do_scalars && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        // loss partials: given already summed over the ranks (tail_in), or summed here over the lists' headers in list order
        float t[4] = {0.f, 0.f, 0.f, 0.f};
        if (tail_in) {
            t[0] = tail_in[0]; t[1] = tail_in[1]; t[2] = tail_in[2]; t[3] = tail_in[3];
        } else {
            for (int r = 0; r < pls.n; ++r) {
                const float *h = pls.l[r].header;
                if (h) { t[0] += h[2]; t[1] += h[3]; t[2] += h[4]; t[3] += h[5]; }
            }
        }
        const float tot[kPartials] = {t[1], t[2], t[3], t[0]};
        scalar_epilogue<!kAdagrad>(tot, k, scalars, scalars, [&](float &gn, float &a, float &b, float dg) {
            if constexpr (kAdagrad) adagrad_elem(gn, a, dg, k.lr, k.eps);
            else OptElem<OPT>::one(gn, a, b, dg, o, nk);
        }, loss_out);
        if (OPT == GLOVE_OPT_NADAM) scalars[4 + (int)(*step & 1)] = nk.sched_new;      // the momentum cache (see nadam_consts)
    }
}

// ------------------------------------------------------------------------------------------
// The sparse Adagrad step for the latency-bound regime (GLOVE_STEP_TAGGED): ONE launch does all the work on the rows — forward,
// gradients AND the Adagrad applies — and a one-workgroup epilogue launch does the once-per-step scalars.  The reference's
// default batch of 1,024 pairs (reference configs/app.ini:39-53) runs the two-launch form as two ramps, a kernel boundary and
// four dependent memory round trips (record -> rows -> partial rows | id record -> partial + table rows -> rows), nothing in
// them is bandwidth; here a chunk is record -> rows -> new row (the chunk walk below, shared with the
// one-launch Adam step).
// What lets one launch both read every row as it was when the step began and update rows: both tables are twinned and
// step-tagged (glove_tables.R_tag / C_tag).  tag[u] = 0, or (1 + step that wrote row u) << 1 | the copy it wrote.  During step t
// a reader takes the copy the tag names unless the tag says "written in step t": then it takes the OTHER copy — the pre-step
// row, which nobody touches during step t.  The writer (the one lane group that owns row u in this step) puts the new row into
// the copy it did not read and then stores the tag.  A racing reader sees the old tag or the new one; either way it is led to
// the pre-step row.  No barrier, no fence, no atomic (a device-scope fence costs 3 - 6 us on this chip: measured).
// The tag is not waited for: the own row and the first trip's partner rows are requested in BOTH copies together with their
// tags (one round trip; the tables of this regime live in the caches) and the copy is chosen in registers.
// ------------------------------------------------------------------------------------------
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct OneSide {
    const int32_t *crec;
    float *own, *own_bias;              // this side's table and bias vector, twinned
    const float *other, *other_bias;    // the partner table, twinned
    float *S1, *S1b;                    // Adagrad accumulators (never twinned: only the id's owner touches them)
    uint64_t *own_tag;
    const uint64_t *other_tag;
    int own_twin, other_twin;           // rows between the two copies
    int n_host, count_index, capP, cap_chunks;
};

// which copy (0 / 1) holds the row as it was when step t began
__device__ inline uint32_t pre_step_copy(uint64_t tag, uint64_t t1 /* 1 + t */) { return (uint32_t)(tag & 1ull) ^ ((tag >> 1) == t1 ? 1u : 0u); }

// A chain record = what one step of a chain leaves for the next: [0] global bias and [1], [2] its slots as they were when the
// step BEGAN, [8 + 4 b ..] the loss partials of its row-side workgroup b.
constexpr int kChainHead = 8;

// ------------------------------------------------------------------------------------------
// The chunk walk of the one-launch kernels (tagged_step_kernel, tagged_adam_kernel), block by block.  An id's chunks are all
// done by the lane group that holds its FIRST chunk, one after the other (the groups that were dealt its other chunks skip
// them): per-chunk sums added in chunk order — for ids up to plan.heavy_chunks chunks the very order of the two-launch form's
// apply, bit for bit — then G = sum + activity-L2 term and the optimizer, expression for expression as the apply launch.  No
// partial rows in memory.  (An id of many chunks is a long serial chain: the forms are for batches whose ids have few chunks —
// GLOVE_STEP_AUTO takes them up to 2,048 pairs.)  Every row-side workgroup leaves its loss partials in the step's chain record.
// The kernels keep what is theirs: which copy of a row they read and write, the slots, the update.  Register arrays travel as
// references of compile-time extent through forced inlining: nothing here may reach scratch.
// ------------------------------------------------------------------------------------------
constexpr int kWalkRecStride = 4 + 3 * kChunkMax + 4;       // dwords of a lane group's record in LDS
template <int LPR> struct WalkPre { static constexpr int value = (1 + 3 * kChunkMax / 4 + LPR - 1) / LPR; };

// The group's first record, requested before anything else: neither the number of chunks is waited for (a plan refilled on the
// device keeps it in memory) nor the global bias (records exist up to the plan's capacity; one that lies behind the side's last
// chunk is dropped unread).  (pre: a native vector type — an array of the struct uint4 went through scratch at four of them.)
template <int LPR>
__device__ __forceinline__ void record_request(u32x4 (&pre)[WalkPre<LPR>::value], const int32_t *crec, int capP, int cap_chunks, int jf, int lg)
{
    const uint4 *rp = reinterpret_cast<const uint4 *>(crec) + (size_t)(jf < cap_chunks ? jf : cap_chunks - 1) * rec_stride_q(capP);
    const int rq0 = 1 + 3 * capP / 4;
#pragma unroll
    for (int x = 0; x < WalkPre<LPR>::value; ++x) {
        const int f = lg + x * LPR;
        pre[x] = reinterpret_cast<const u32x4 *>(rp)[rec_gq(f < rq0 ? f : 0)];
    }
}

// Record j (descriptor + pair fields) in contiguous 16-B loads -> LDS as is: a round trip of its own
template <int LPR>
__device__ __forceinline__ void record_fetch(uint32_t *rec, const int32_t *crec, int j, int sq, int rq, int lg)
{
    const uint4 *rp = reinterpret_cast<const uint4 *>(crec) + (size_t)j * sq;
    uint4 *lrec = reinterpret_cast<uint4 *>(rec);
    for (int f = lg; f < rq; f += LPR) lrec[f] = rp[rec_gq(f)];
}

// ... the record a group begins with: the one requested at the kernel's start on its first round, from memory afterwards
template <int LPR>
__device__ __forceinline__ void record_first(uint32_t *rec, const u32x4 (&pre)[WalkPre<LPR>::value], bool requested, const int32_t *crec,
                                             int j0, int sq, int rq, int lg)
{
    if (requested) {
#pragma unroll
        for (int x = 0; x < WalkPre<LPR>::value; ++x) {
            const int f = lg + x * LPR;
            if (f < rq) reinterpret_cast<u32x4 *>(rec)[f] = pre[x];
        }
    } else {
        record_fetch<LPR>(rec, crec, j0, sq, rq, lg);
    }
}

// {id, pairs, position of the id, first-chunk flag | chunks behind} (the same wave wrote it: LDS ops of one wave complete in order)
__device__ __forceinline__ uint4 record_header(const uint32_t *rec) { return *reinterpret_cast<const uint4 *>(rec); }

// Pairs q0 .. q0 + U - 1 of the record in LDS: partner row numbers (other_add: rows to the copy the step reads, where the whole
// table has one), 2 w / B and y
template <int U>
__device__ __forceinline__ void unpack_pairs(const uint32_t *rec, int q0, uint32_t other_add, float inv_batch, int32_t (&col)[U],
                                             float (&w2)[U], float (&yq)[U])
{
#pragma unroll
    for (int a4 = 0; a4 < U; a4 += 4) {
        const int rp0 = rec_pair(q0 + a4);
        const uint4 pc = *reinterpret_cast<const uint4 *>(&rec[rp0]);
        const uint4 pw = *reinterpret_cast<const uint4 *>(&rec[rp0 + kRecPad]);
        const uint4 py = *reinterpret_cast<const uint4 *>(&rec[rp0 + 2 * kRecPad]);
        col[a4] = (int32_t)(pc.x + other_add); col[a4 + 1] = (int32_t)(pc.y + other_add);
        col[a4 + 2] = (int32_t)(pc.z + other_add); col[a4 + 3] = (int32_t)(pc.w + other_add);
        const float sc2 = 2.0f * inv_batch;
        w2[a4] = sc2 * __uint_as_float(pw.x); w2[a4 + 1] = sc2 * __uint_as_float(pw.y);
        w2[a4 + 2] = sc2 * __uint_as_float(pw.z); w2[a4 + 3] = sc2 * __uint_as_float(pw.w);
        yq[a4] = __uint_as_float(py.x); yq[a4 + 1] = __uint_as_float(py.y);
        yq[a4 + 2] = __uint_as_float(py.z); yq[a4 + 3] = __uint_as_float(py.w);
    }
}

// The partner rows of a trip whose row numbers are final, and their biases (lane 0 of the group; through the byte offset)
template <int LPR, int NV, bool FULL, int U>
__device__ __forceinline__ void gather_partners(f4 (&c)[U][NV], float (&bcv)[U], const float *other, const float *other_bias,
                                                const int32_t (&col)[U], int d4, int lg)
{
#pragma unroll
    for (int a = 0; a < U; ++a) {
        load_row_fast<LPR, NV, FULL>(c[a], other, col[a], d4, lg);
        bcv[a] = 0.f;
        if (lg == 0) bcv[a] = *reinterpret_cast<const float *>(reinterpret_cast<const char *>(other_bias) + (uint32_t)col[a] * 4u);
    }
}

// One trip: U pairs' dot products, summed over the lane group, through the head into the chunk's sums
template <int LPR, int NV, int U>
__device__ __forceinline__ void walk_trip(const f4 (&r)[NV], const f4 (&c)[U][NV], const float (&bcv)[U], const float (&w2)[U],
                                          const float (&yq)[U], int q0, int n, float bg, int head, float inv_batch, float neg_factor,
                                          f4 (&acc)[NV], float &se_c, float &cc_sum, float &bsq, float &ed)
{
    float dp[U], cc[U];
#pragma unroll
    for (int a = 0; a < U; ++a) {
        dp[a] = 0.f; cc[a] = 0.f;
#pragma unroll
        for (int k = 0; k < NV; ++k) { dp[a] += dot4(r[k], c[a][k]); cc[a] += dot4(c[a][k], c[a][k]); }
        dp[a] += bcv[a];
    }
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
#pragma unroll
    for (int a = 0; a < U; ++a) {
        const float valid = (q0 + a < n) ? 1.0f : 0.f;
        float e;
        if (head == GLOVE_HEAD_REGRESSION) {
            const float diff = (dp[a] + bg) - yq[a];
            e = w2[a] * diff;
            ed += e * diff;
        } else {
            const float p = dp[a] + bg;
            const float en = expf(-fabsf(p));
            const float s = (p >= 0.f ? 1.0f : en) / (1.0f + en);
            const float lse = log1pf(en);
            const float wn = 2.0f * inv_batch * neg_factor * valid * yq[a];
            e = 0.5f * (w2[a] * (s - 1.0f) + wn * s);
            ed += w2[a] * (fmaxf(-p, 0.f) + lse) + wn * (fmaxf(p, 0.f) + lse);
        }
#pragma unroll
        for (int k = 0; k < NV; ++k) acc[k] += e * c[a][k];
        se_c += e;
        cc_sum += valid * cc[a];
        bsq += valid * bcv[a] * bcv[a];
    }
}

// A chunk is done: the row side's loss partials, and the id's sums in chunk order (the first chunk's taken as they are, like
// the apply launch's traversal)
template <int NV>
__device__ __forceinline__ void chunk_close(bool is_row, bool first, int n, int lg, const f4 (&r)[NV], float own_b, const f4 (&acc)[NV],
                                            float se_c, float cc_sum, float bsq, float ed, float (&part)[kPartials], f4 (&G)[NV], float &Gb)
{
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
    if (first) {
#pragma unroll
        for (int k = 0; k < NV; ++k) G[k] = acc[k];
        Gb = se_c;
    } else {
#pragma unroll
        for (int k = 0; k < NV; ++k) G[k] += acc[k];
        Gb += se_c;
    }
}

// G = summed gradient + activity-L2 term (for_each_id, expression for expression)
template <int NV>
__device__ __forceinline__ void add_activity_l2(f4 (&G)[NV], float &Gb, const f4 (&r)[NV], float bval, int pairs, const StepConsts &kc)
{
    const float cnt = (float)pairs;
    const float kcn = kc.kappa * cnt;
#pragma unroll
    for (int k = 0; k < NV; ++k) G[k] += kcn * r[k];
    Gb += kc.kappa_b * cnt * bval;
}

// The workgroup's loss partials into the step's chain record (row side only)
__device__ __forceinline__ void walk_partials_store(bool is_row, float (&part)[kPartials], float inv_batch, float *blockpart)
{
    if (is_row) {
        part[0] *= 0.5f / inv_batch;        // sum e diff = 2 inv_batch sum w diff^2
        block_partials_store(part, blockpart);
    }
}

// The global bias of THIS step.  The one thing a step needs of ALL pairs of the step before is sum e (the global bias'
// gradient): a grid-wide reduction.  Instead of a launch (or a device-scope fence: 3 - 6 us) between the steps of a chain, every
// workgroup of step i derives the bias itself — from the bias step i - 1 began with (and its slots: Adagrad's accumulator, or
// Adam's m and v with the step t - 1 that lr_t needs) and the loss partials its row-side workgroups left (prev), summed in the
// fixed order of the two-launch form: same bits in every workgroup — and leaves what it began with in a record of its own
// (mine), which nobody of this launch reads.  A chain's first step takes the bias from the tables' scalars.
template <int OPT>
__device__ __forceinline__ float chain_bias(const float *__restrict__ prev, int prev_blocks, const float *__restrict__ scalars,
                                            float *__restrict__ mine, const StepConsts &kc, float b1, float b2, double ln_beta1,
                                            double ln_beta2, int64_t t)
{
    constexpr bool kAdam = OPT == GLOVE_OPT_ADAM;
    __shared__ float s_g[kAdam ? 3 : 2];
    if (prev) {
        float tot[kPartials];
        sum_blockpart(prev + kChainHead, prev_blocks, tot);
        if (threadIdx.x == 0) {
            const float g0 = prev[0];
            const float dg = tot[3] + 2.0f * kc.m * kc.l2 * g0;
            float gn = g0, s1 = prev[1];
            if constexpr (kAdam) {
                float s2 = prev[2];
                adam_elem(gn, s1, s2, dg, adam_lr_t(kc.lr, ln_beta1, ln_beta2, t - 1), b1, b2, kc.eps);
                s_g[2] = s2;
            } else {
                adagrad_elem(gn, s1, dg, kc.lr, kc.eps);
            }
            s_g[0] = gn; s_g[1] = s1;
        }
    } else if (threadIdx.x == 0) {
        s_g[0] = scalars[0]; s_g[1] = scalars[1];
        if constexpr (kAdam) s_g[2] = scalars[2];
    }
    __syncthreads();
    const float g = s_g[0];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        mine[0] = g; mine[1] = s_g[1];
        if constexpr (kAdam) mine[2] = s_g[2];
    }
    return g;
}

template <int LPR, int NV, bool FULL>
__global__ __launch_bounds__(kBlock, NV <= 2 ? 2 : 1) void tagged_step_kernel(
    const int32_t *__restrict__ counts, OneSide rowside, OneSide colside, int row_blocks, const float *__restrict__ scalars,
    const int64_t *__restrict__ step, int d4, float inv_batch, int head, float neg_factor, StepConsts kc,
    const float *__restrict__ prev, int prev_blocks, float *__restrict__ mine, int chain_i)
{
    constexpr int GPB = kBlock / LPR;
    constexpr int U = PassUnroll<NV>::value;
    __shared__ __attribute__((aligned(16))) uint32_t fld_raw[GPB * kWalkRecStride];
    uint32_t *rec = fld_raw + (threadIdx.x / LPR) * kWalkRecStride;
    const int lg = threadIdx.x % LPR, grp = threadIdx.x / LPR;
    const bool is_row = (int)blockIdx.x < row_blocks;
    const OneSide &sd = is_row ? rowside : colside;
    const int bid = is_row ? blockIdx.x : blockIdx.x - row_blocks;
    const int nblk = is_row ? row_blocks : gridDim.x - row_blocks;
    u32x4 pre[WalkPre<LPR>::value];
    record_request<LPR>(pre, sd.crec, sd.capP, sd.cap_chunks, bid * GPB + grp, lg);
    const int n_chunks = sd.n_host >= 0 ? sd.n_host : counts[sd.count_index];
    // global_step stands still during a chain (its last launch's epilogue advances it): this is step *step + chain_i
    const uint64_t t1 = (uint64_t)(*step) + (uint64_t)chain_i + 1ull;
    float part[kPartials] = {0.f, 0.f, 0.f, 0.f};
    const int capP = sd.capP;
    const int rq = 1 + 3 * capP / 4;
    const int sq = rec_stride_q(capP);
    const float g = chain_bias<GLOVE_OPT_ADAGRAD>(prev, prev_blocks, scalars, mine, kc, 0.f, 0.f, 0.0, 0.0, 0);
    float *blockpart = mine + kChainHead;

    for (int j0 = bid * GPB + grp; j0 < n_chunks; j0 += nblk * GPB) {
        // ---- round trip 1: the record
        record_first<LPR>(rec, pre, j0 == bid * GPB + grp, sd.crec, j0, sq, rq, lg);
        uint4 hdr = record_header(rec);
        if (!(hdr.w >> 31)) continue;                           // not the first chunk of its id: the group that holds the first one does it
        const int32_t u = (int32_t)hdr.x;
        const int chunks = 1 + (int)(hdr.w & 0x7fffffffu);
        // ---- round trip 2: the own row in both copies, its tag, the accumulator (and, below, the first trip's partner rows)
        f4 r[NV], r1[NV], A[NV], G[NV];
        load_row<LPR, NV>(r, sd.own, u, d4, lg);
        load_row<LPR, NV>(r1, sd.own, u + sd.own_twin, d4, lg);
        const uint64_t own_tg = sd.own_tag[u];
        const float ob0 = sd.own_bias[u], ob1 = sd.own_bias[u + sd.own_twin];
        load_row<LPR, NV>(A, sd.S1, u, d4, lg);
        float Ab = sd.S1b[u];
#pragma unroll
        for (int k = 0; k < NV; ++k) G[k] = f4{0.f, 0.f, 0.f, 0.f};
        float Gb = 0.f, own_b = 0.f, bg = 0.f;
        uint32_t own_copy = 0;
        int pairs = 0;
        for (int ch = 0; ch < chunks; ++ch) {
            if (ch > 0) {                                       // the id's next chunk
                record_fetch<LPR>(rec, sd.crec, j0 + ch, sq, rq, lg);
                hdr = record_header(rec);
            }
            const int n = (int)hdr.y;
            pairs += n;
            // the tags of all partners of the chunk: lane t looks pair t's up and leaves the row that is current in the record
            // (consumed from the second trip on; the first trip does not wait for it)
            uint64_t ptag[(kChunkMax + LPR - 1) / LPR];
#pragma unroll
            for (int x = 0; x < (kChunkMax + LPR - 1) / LPR; ++x) {
                const int t = lg + x * LPR;
                ptag[x] = t < n ? sd.other_tag[rec[rec_pair(t)]] : 0ull;
            }
            f4 acc[NV];
#pragma unroll
            for (int k = 0; k < NV; ++k) acc[k] = f4{0.f, 0.f, 0.f, 0.f};
            float se_c = 0.f, cc_sum = 0.f, bsq = 0.f, ed = 0.f;
            for (int q0 = 0; q0 < n; q0 += U) {
                int32_t col[U];
                float w2[U], yq[U];
                unpack_pairs<U>(rec, q0, 0u, inv_batch, col, w2, yq);
                f4 c[U][NV];
                float bcv[U];
                if (q0 == 0) {
                    // first trip: both copies of every partner row travel with the tags; the choice happens in registers
                    f4 c1[U][NV];
                    float b0[U], b1[U];
#pragma unroll
                    for (int a = 0; a < U; ++a) {
                        load_row_fast<LPR, NV, FULL>(c[a], sd.other, col[a], d4, lg);
                        load_row_fast<LPR, NV, FULL>(c1[a], sd.other, col[a] + sd.other_twin, d4, lg);
                        b0[a] = b1[a] = 0.f;
                        if (lg == 0) {
                            b0[a] = sd.other_bias[col[a]];
                            b1[a] = sd.other_bias[col[a] + sd.other_twin];
                        }
                    }
                    if (ch == 0) {                              // (the own row's copy: known with this trip)
                        own_copy = pre_step_copy(own_tg, t1);
#pragma unroll
                        for (int k = 0; k < NV; ++k) r[k] = own_copy ? r1[k] : r[k];
                        own_b = own_copy ? ob1 : ob0;
                        bg = own_b + g;
                    }
                    // the partners' tags, handed round: pair a of this trip was looked up by lane a % LPR (slot a / LPR)
#pragma unroll
                    for (int a = 0; a < U; ++a) {
                        const uint64_t tg = __shfl(ptag[a / LPR], (int)((threadIdx.x & 63) / LPR * LPR + a % LPR), 64);
                        const bool second = pre_step_copy(tg, t1) != 0;
#pragma unroll
                        for (int k = 0; k < NV; ++k) c[a][k] = second ? c1[a][k] : c[a][k];
                        bcv[a] = second ? b1[a] : b0[a];
                    }
                    // later trips read the current row straight away: the record's ids become row numbers
#pragma unroll
                    for (int x = 0; x < (kChunkMax + LPR - 1) / LPR; ++x) {
                        const int t = lg + x * LPR;
                        if (t < n && t >= U) rec[rec_pair(t)] += pre_step_copy(ptag[x], t1) ? (uint32_t)sd.other_twin : 0u;
                    }
                } else {
                    gather_partners<LPR, NV, FULL, U>(c, bcv, sd.other, sd.other_bias, col, d4, lg);
                }
                walk_trip<LPR, NV, U>(r, c, bcv, w2, yq, q0, n, bg, head, inv_batch, neg_factor, acc, se_c, cc_sum, bsq, ed);
            }
            chunk_close<NV>(is_row, ch == 0, n, lg, r, own_b, acc, se_c, cc_sum, bsq, ed, part, G, Gb);
        }
        // ---- Adagrad (AdagradApply, expression for expression) into the copy nobody reads during this step, then the tag
        {
            float bval = own_b;
            add_activity_l2<NV>(G, Gb, r, bval, pairs, kc);
#pragma unroll
            for (int k = 0; k < NV; ++k) adagrad_vec(r[k], A[k], G[k], kc.lr, kc.eps);
            store_row<LPR, NV>(sd.S1, (size_t)u, d4, lg, A);
            const int32_t new_at = u + (own_copy ? 0 : sd.own_twin);
            store_row<LPR, NV>(sd.own, (size_t)new_at, d4, lg, r);
            if (lg == 0) {
                adagrad_elem(bval, Ab, Gb, kc.lr, kc.eps);
                sd.S1b[u] = Ab;
                sd.own_bias[new_at] = bval;
                sd.own_tag[u] = t1 << 1 | (uint64_t)(own_copy ^ 1u);
            }
        }
    }
    walk_partials_store(is_row, part, inv_batch, blockpart);
}

// ------------------------------------------------------------------------------------------
// Keras-legacy Adam in ONE launch per step (the reference's default optimizer at its default batch: configs/app.ini:39-53),
// on twinned tables.  The legacy optimizer's sparse path rewrites EVERY row every step (m *= b1, v *= b2, var -= lr_t
// m / (sqrt(v) + eps) over the whole table, a11), so the twin needs no tags: a step reads copy c of both tables and writes
// copy 1 - c of both, all rows — the batch's rows by the chunk walk above (gradient, then Adam), every other row by a sweep
// that finds the batch's ids in the plan's bitmaps (glove_plan.r_mark / c_mark) and leaves them alone.  scalars[3] says which
// copy is current between chains.  The global bias travels through chain records ([0] bias, [1] m, [2] v as the step began).
// ------------------------------------------------------------------------------------------
// ... in tagged_adam_kernel: four where the registers allow (d = 64: 10.8 -> 10.2 us per step; six spill: 14.2)
constexpr int tagged_sweep_rows(int nv) { return nv <= 2 ? 4 : 2; }

struct AdamSide {
    const int32_t *crec;
    float *own, *own_bias;              // this side's table and bias vector, twinned
    const float *other, *other_bias;    // the partner table, twinned
    float *S1, *S1b, *S2, *S2b;         // m and v (never twinned: only the row's owner or sweeper touches them)
    const uint32_t *mark;               // bitmap of the batch's ids of this side
    int own_twin, other_twin;           // rows between the two copies = rows of the table
    int n_host, count_index, capP, cap_chunks;
};

template <int LPR, int NV, bool FULL>
__global__ __launch_bounds__(kBlock, NV <= 2 ? 2 : 1) void tagged_adam_kernel(
    const int32_t *__restrict__ counts, AdamSide rowside, AdamSide colside, int row_blocks, int chunk_blocks,
    const float *__restrict__ scalars, const int64_t *__restrict__ step, int d4, float inv_batch, int head, float neg_factor,
    StepConsts kc, float b1, float b2, double ln_beta1, double ln_beta2, const float *__restrict__ prev, int prev_blocks,
    float *__restrict__ mine, int chain_i)
{
    constexpr int GPB = kBlock / LPR;
    constexpr int kRows = tagged_sweep_rows(NV);
    const int lg = threadIdx.x % LPR, grp = threadIdx.x / LPR;
    const uint32_t cur = (scalars[3] != 0.f ? 1u : 0u) ^ (uint32_t)(chain_i & 1);     // the copy this step reads (scalars[3]: as the chain began)
    const int64_t t = *step + chain_i + 1;                                            // global_step stands still during a chain
    const float lr_t = adam_lr_t(kc.lr, ln_beta1, ln_beta2, t);
    if ((int)blockIdx.x >= chunk_blocks) {
        // ---- sweep: a lane group per table row (R's rows first, then C's), kRows rows in flight; the batch's rows belong
        // to the chunk groups
        const int sb0 = blockIdx.x - chunk_blocks, nsb = gridDim.x - chunk_blocks;
        const int Vr = rowside.own_twin, Vc = colside.own_twin;
        const int total = Vr + Vc, stride = nsb * GPB;
        for (int v0 = sb0 * GPB + grp; v0 < total; v0 += kRows * stride) {
            f4 Wv[kRows][NV], M[kRows][NV], Vv[kRows][NV];
            float bval[kRows], Mb[kRows], Vb[kRows];
            uint32_t mk[kRows];
#pragma unroll
            for (int r = 0; r < kRows; ++r) {
                const int v = v0 + r * stride;
                const bool live = v < total, is_row = v < Vr;
                const int id = live ? (is_row ? v : v - Vr) : 0;
                const AdamSide &sd = is_row ? rowside : colside;
                mk[r] = live ? (sd.mark[id >> 5] >> (id & 31)) & 1u : 1u;
                const int at = id + (cur ? sd.own_twin : 0);
                load_row<LPR, NV>(Wv[r], sd.own, at, d4, lg);
                load_row<LPR, NV>(M[r], sd.S1, id, d4, lg);
                load_row<LPR, NV>(Vv[r], sd.S2, id, d4, lg);
                bval[r] = Mb[r] = Vb[r] = 0.f;
                if (lg == 0) { bval[r] = sd.own_bias[at]; Mb[r] = sd.S1b[id]; Vb[r] = sd.S2b[id]; }
            }
#pragma unroll
            for (int r = 0; r < kRows; ++r) {
                const int v = v0 + r * stride;
                if (v >= total || mk[r]) continue;
                const bool is_row = v < Vr;
                const int id = is_row ? v : v - Vr;
                const AdamSide &sd = is_row ? rowside : colside;
                const f4 zero = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kk = 0; kk < NV; ++kk) adam_vec(Wv[r][kk], M[r][kk], Vv[r][kk], zero, lr_t, b1, b2, kc.eps);
                const int to = id + (cur ? 0 : sd.own_twin);
                store_row<LPR, NV>(sd.S1, (size_t)id, d4, lg, M[r]);
                store_row<LPR, NV>(sd.S2, (size_t)id, d4, lg, Vv[r]);
                store_row<LPR, NV>(sd.own, (size_t)to, d4, lg, Wv[r]);
                if (lg == 0) {
                    adam_elem(bval[r], Mb[r], Vb[r], 0.f, lr_t, b1, b2, kc.eps);
                    sd.S1b[id] = Mb[r];
                    sd.S2b[id] = Vb[r];
                    sd.own_bias[to] = bval[r];
                }
            }
        }
        return;
    }
    constexpr int U = PassUnroll<NV>::value;
    __shared__ __attribute__((aligned(16))) uint32_t fld_raw[GPB * kWalkRecStride];
    uint32_t *rec = fld_raw + (threadIdx.x / LPR) * kWalkRecStride;
    const bool is_row = (int)blockIdx.x < row_blocks;
    const AdamSide &sd = is_row ? rowside : colside;
    const int bid = is_row ? blockIdx.x : blockIdx.x - row_blocks;
    const int nblk = is_row ? row_blocks : chunk_blocks - row_blocks;
    u32x4 pre[WalkPre<LPR>::value];
    record_request<LPR>(pre, sd.crec, sd.capP, sd.cap_chunks, bid * GPB + grp, lg);
    const int n_chunks = sd.n_host >= 0 ? sd.n_host : counts[sd.count_index];
    float part[kPartials] = {0.f, 0.f, 0.f, 0.f};
    const int capP = sd.capP;
    const int rq = 1 + 3 * capP / 4;
    const int sq = rec_stride_q(capP);
    const float g = chain_bias<GLOVE_OPT_ADAM>(prev, prev_blocks, scalars, mine, kc, b1, b2, ln_beta1, ln_beta2, t);
    float *blockpart = mine + kChainHead;
    const uint32_t other_add = cur ? (uint32_t)sd.other_twin : 0u;

    for (int j0 = bid * GPB + grp; j0 < n_chunks; j0 += nblk * GPB) {
        record_first<LPR>(rec, pre, j0 == bid * GPB + grp, sd.crec, j0, sq, rq, lg);
        uint4 hdr = record_header(rec);
        if (!(hdr.w >> 31)) continue;                           // the group that holds the id's first chunk does the whole id
        const int32_t u = (int32_t)hdr.x;
        const int chunks = 1 + (int)(hdr.w & 0x7fffffffu);
        const int32_t own_at = u + (cur ? sd.own_twin : 0);
        f4 r[NV], M[NV], Vv[NV], G[NV];
        load_row<LPR, NV>(r, sd.own, own_at, d4, lg);
        const float own_b = sd.own_bias[own_at];
        load_row<LPR, NV>(M, sd.S1, u, d4, lg);
        load_row<LPR, NV>(Vv, sd.S2, u, d4, lg);
        float Mb = sd.S1b[u], Vb = sd.S2b[u];
        const float bg = own_b + g;
#pragma unroll
        for (int k = 0; k < NV; ++k) G[k] = f4{0.f, 0.f, 0.f, 0.f};
        float Gb = 0.f;
        int pairs = 0;
        for (int ch = 0; ch < chunks; ++ch) {
            if (ch > 0) {
                record_fetch<LPR>(rec, sd.crec, j0 + ch, sq, rq, lg);
                hdr = record_header(rec);
            }
            const int n = (int)hdr.y;
            pairs += n;
            f4 acc[NV];
#pragma unroll
            for (int k = 0; k < NV; ++k) acc[k] = f4{0.f, 0.f, 0.f, 0.f};
            float se_c = 0.f, cc_sum = 0.f, bsq = 0.f, ed = 0.f;
            for (int q0 = 0; q0 < n; q0 += U) {
                int32_t col[U];
                float w2[U], yq[U];
                unpack_pairs<U>(rec, q0, other_add, inv_batch, col, w2, yq);
                f4 c[U][NV];
                float bcv[U];
                gather_partners<LPR, NV, FULL, U>(c, bcv, sd.other, sd.other_bias, col, d4, lg);
                walk_trip<LPR, NV, U>(r, c, bcv, w2, yq, q0, n, bg, head, inv_batch, neg_factor, acc, se_c, cc_sum, bsq, ed);
            }
            chunk_close<NV>(is_row, ch == 0, n, lg, r, own_b, acc, se_c, cc_sum, bsq, ed, part, G, Gb);
        }
        {
            float bval = own_b;
            add_activity_l2<NV>(G, Gb, r, bval, pairs, kc);
#pragma unroll
            for (int k = 0; k < NV; ++k) adam_vec(r[k], M[k], Vv[k], G[k], lr_t, b1, b2, kc.eps);
            store_row<LPR, NV>(sd.S1, (size_t)u, d4, lg, M);
            store_row<LPR, NV>(sd.S2, (size_t)u, d4, lg, Vv);
            const int32_t new_at = u + (cur ? 0 : sd.own_twin);
            store_row<LPR, NV>(sd.own, (size_t)new_at, d4, lg, r);
            if (lg == 0) {
                adam_elem(bval, Mb, Vb, Gb, lr_t, b1, b2, kc.eps);
                sd.S1b[u] = Mb;
                sd.S2b[u] = Vb;
                sd.own_bias[new_at] = bval;
            }
        }
    }
    walk_partials_store(is_row, part, inv_batch, blockpart);
}

// The end of a chain of n one-launch steps: the last step's loss partials -> the loss scalars and the global bias the NEXT step
// begins with, into the tables; global_step advances by n (Adam: and scalars[3] says which copy is current).  One workgroup.
template <int OPT>
__global__ __launch_bounds__(kBlock) void tagged_flush_kernel(float *__restrict__ scalars, int64_t *__restrict__ step,
                                                              const float *__restrict__ last, int nblocks, int n, StepConsts k,
                                                              float b1, float b2, double ln_beta1, double ln_beta2,
                                                              float *__restrict__ loss_out)
{
    float tot[kPartials];
    sum_blockpart(last + kChainHead, nblocks, tot);
    if (threadIdx.x == 0) {
        if (OPT == GLOVE_OPT_ADAM) {
            scalar_epilogue<true>(tot, k, last, scalars, [&](float &gn, float &Mg, float &Vg, float dg) {
                adam_elem(gn, Mg, Vg, dg, adam_lr_t(k.lr, ln_beta1, ln_beta2, *step + n), b1, b2, k.eps);
            }, loss_out);
            if (n & 1) scalars[3] = scalars[3] != 0.f ? 0.f : 1.0f;
        } else {
            scalar_epilogue<false>(tot, k, last, scalars, [&](float &gn, float &Ag, float &, float dg) { adagrad_elem(gn, Ag, dg, k.lr, k.eps); },
                                   loss_out);
        }
        *step += n;
    }
}

// Twinned tables whose second copies are current as a whole (the one-launch Adam step, scalars[3] != 0): every row home
template <int LPR, int NV>
__global__ __launch_bounds__(kBlock) void twin_home_kernel(float *__restrict__ W, float *__restrict__ bias, const float *__restrict__ scalars,
                                                           int V, int d4)
{
    if (scalars[3] == 0.f) return;
    constexpr int GPB = kBlock / LPR;
    const int lg = threadIdx.x % LPR, grp = threadIdx.x / LPR;
    for (int u = blockIdx.x * GPB + grp; u < V; u += gridDim.x * GPB) {
        f4 v[NV];
        load_row<LPR, NV>(v, W, u + V, d4, lg);
        store_row<LPR, NV>(W, (size_t)u, d4, lg, v);
        if (lg == 0) bias[u] = bias[u + V];
    }
}

__global__ void twin_home_done_kernel(float *scalars) { if (threadIdx.x == 0 && blockIdx.x == 0) scalars[3] = 0.f; }

// Step-tagged twinned tables back to the plain form: rows whose current copy is the second one are copied home, tags cleared
template <int LPR, int NV>
__global__ __launch_bounds__(kBlock) void untag_kernel(float *__restrict__ W, float *__restrict__ bias, uint64_t *__restrict__ tag,
                                                       int V, int d4)
{
    constexpr int GPB = kBlock / LPR;
    const int lg = threadIdx.x % LPR, grp = threadIdx.x / LPR;
    for (int u = blockIdx.x * GPB + grp; u < V; u += gridDim.x * GPB) {
        const uint64_t tg = tag[u];
        if (tg == 0) continue;
        if (tg & 1ull) {
            f4 v[NV];
            load_row<LPR, NV>(v, W, u + V, d4, lg);
            store_row<LPR, NV>(W, (size_t)u, d4, lg, v);
            if (lg == 0) bias[u] = bias[u + V];
        }
        if (lg == 0) tag[u] = 0;
    }
}

// Twinned row table back to its plain form: every row whose current copy is the second one is copied into the first,
// all versions become 0.  Everything but the fused twin step expects this form.
template <int LPR, int NV>
__global__ __launch_bounds__(kBlock) void canonicalize_kernel(float *__restrict__ R, float *__restrict__ br,
                                                              uint8_t *__restrict__ ver, int V_row, int d4)
{
    constexpr int GPB = kBlock / LPR;
    const int lg = threadIdx.x % LPR, grp = threadIdx.x / LPR;
    for (int u = blockIdx.x * GPB + grp; u < V_row; u += gridDim.x * GPB) {
        if (!ver[u]) continue;
        f4 v[NV];
        load_row<LPR, NV>(v, R, u + V_row, d4, lg);
        store_row<LPR, NV>(R, (size_t)u, d4, lg, v);
        if (lg == 0) { br[u] = br[u + V_row]; ver[u] = 0; }
    }
}

// rows[i] = W[ids[i]] (d floats each), biases[i] = bias[ids[i]]: what the owner of a table shard sends to the ranks
// whose batches touch those rows
template <int LPR, int NV>
__global__ __launch_bounds__(kBlock) void gather_rows_kernel(
    const float *__restrict__ W, const float *__restrict__ bias, const int32_t *__restrict__ ids, int n, int d4,
    float *__restrict__ rows, float *__restrict__ biases)
{
    constexpr int GPB = kBlock / LPR;
    const int lg = threadIdx.x % LPR, grp = threadIdx.x / LPR;
    for (int i = blockIdx.x * GPB + grp; i < n; i += gridDim.x * GPB) {
        const int32_t id = ids[i];
        f4 v[NV];
        load_row<LPR, NV>(v, W, id, d4, lg);
        store_row<LPR, NV>(rows, (size_t)i, d4, lg, v);
        if (lg == 0) biases[i] = bias[id];
    }
}

// ------------------------------------------------------------------------------------------
// Dense sweeps over [R | C | br | bc] consuming (and zeroing) G_flat.
// ------------------------------------------------------------------------------------------
struct DenseSeg { float *W, *S1, *S2, *G; int64_t n; };
struct DenseSegs { DenseSeg s[4]; };

__global__ __launch_bounds__(kBlock) void dense_adagrad_kernel(
    DenseSegs segs, StepConsts k, float *__restrict__ scalars, float *__restrict__ tail,
    float *__restrict__ loss_out, int do_scalars)
{
    // segments 0,1 = [V,d] tables (float4 body); 2,3 = bias vectors, whose G pointers are only 16-B
    // aligned when V % 4 == 0 and which are tiny: swept scalar by the same launch
    const DenseSeg sg = segs.s[blockIdx.y];
    const int64_t n4 = blockIdx.y < 2 ? sg.n / 4 : 0;
    f4 *W4 = reinterpret_cast<f4 *>(sg.W), *A4 = reinterpret_cast<f4 *>(sg.S1), *G4 = reinterpret_cast<f4 *>(sg.G);
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kBlock) {
        const f4 gv = G4[i];
        if (gv.x == 0.f && gv.y == 0.f && gv.z == 0.f && gv.w == 0.f) continue;  // untouched: exact no-op
        f4 a = A4[i], wv = W4[i];
        adagrad_vec(wv, a, gv, k.lr, k.eps);
        A4[i] = a; W4[i] = wv; G4[i] = f4{0.f, 0.f, 0.f, 0.f};
    }
    for (int64_t i = n4 * 4 + (int64_t)blockIdx.x * kBlock + threadIdx.x; i < sg.n; i += (int64_t)gridDim.x * kBlock) {
        const float gv = sg.G[i];
        if (gv != 0.f) { adagrad_elem(sg.W[i], sg.S1[i], gv, k.lr, k.eps); sg.G[i] = 0.f; }
    }
    if (do_scalars && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        const float g = scalars[0];
        const float tot[kPartials] = {tail[1], tail[2], tail[3], tail[0]};
        float loss, L, reg;
        loss_from_partials(tot, k, g, loss, L, reg);
        const float dg = tail[0] + 2.0f * k.m * k.l2 * g;
        adagrad_elem(scalars[0], scalars[1], dg, k.lr, k.eps);
        if (loss_out) { loss_out[0] = loss; loss_out[1] = L; loss_out[2] = reg; loss_out[3] = tail[0]; }
        tail[0] = tail[1] = tail[2] = tail[3] = 0.f;
    }
}

__global__ __launch_bounds__(kBlock) void dense_adam_kernel(
    DenseSegs segs, StepConsts k, float b1, float b2, double ln_beta1, double ln_beta2, const int64_t *__restrict__ step,
    float *__restrict__ scalars, float *__restrict__ tail, float *__restrict__ loss_out, int do_scalars)
{
    const DenseSeg sg = segs.s[blockIdx.y];
    // t = global_step after rowpass advanced it; lr_t = lr sqrt(1-b2^t)/(1-b1^t)  (Keras legacy Adam)
    // 1 - beta^t = -expm1(t ln beta): the logs come from the host in fp64, so each wave pays two fp64
    // multiplies and two expm1f instead of two fp64 pow() (~290 fp64 instructions, a third of this kernel's time)
    const float lr_t = adam_lr_t(k.lr, ln_beta1, ln_beta2, *step);
    const int64_t n4 = blockIdx.y < 2 ? sg.n / 4 : 0;
    f4 *W4 = reinterpret_cast<f4 *>(sg.W), *M4 = reinterpret_cast<f4 *>(sg.S1), *V4 = reinterpret_cast<f4 *>(sg.S2),
       *G4 = reinterpret_cast<f4 *>(sg.G);
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kBlock) {
        const f4 gv = G4[i];
        f4 m = M4[i], v = V4[i], wv = W4[i];
        adam_vec(wv, m, v, gv, lr_t, b1, b2, k.eps);
        M4[i] = m; V4[i] = v; W4[i] = wv;
        if (gv.x != 0.f || gv.y != 0.f || gv.z != 0.f || gv.w != 0.f) G4[i] = f4{0.f, 0.f, 0.f, 0.f};
    }
    for (int64_t i = n4 * 4 + (int64_t)blockIdx.x * kBlock + threadIdx.x; i < sg.n; i += (int64_t)gridDim.x * kBlock) {
        adam_elem(sg.W[i], sg.S1[i], sg.S2[i], sg.G[i], lr_t, b1, b2, k.eps);
        sg.G[i] = 0.f;
    }
    if (do_scalars && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        const float g = scalars[0];
        const float tot[kPartials] = {tail[1], tail[2], tail[3], tail[0]};
        float loss, L, reg;
        loss_from_partials(tot, k, g, loss, L, reg);
        const float dg = tail[0] + 2.0f * k.m * k.l2 * g;
        adam_elem(scalars[0], scalars[1], scalars[2], dg, lr_t, b1, b2, k.eps);
        if (loss_out) { loss_out[0] = loss; loss_out[1] = L; loss_out[2] = reg; loss_out[3] = tail[0]; }
        tail[0] = tail[1] = tail[2] = tail[3] = 0.f;
    }
}


// ------------------------------------------------------------------------------------------
// The other Keras optimizers `tf.keras.optimizers.get(name)` resolves (reference src/models/train_utils.py:13-16), as apply
// epilogues on the same traversal as AdagradApply.  Semantics: include/glove_hip.h glove_hyper.optimizer; restated in
// oracle/glove_ref.py (_sgd, _rmsprop_dense_decay, _adamax).  LazyAdam (GLOVE_OPT_LAZYADAM, this build's addition: Adam's update
// on the touched rows alone) and RowWiseAdagrad (GLOVE_OPT_ROWWISE_ADAGRAD: one accumulator per embedding row, fed by the row's
// mean squared gradient) are the epilogues here that are no Keras-legacy names; restated in tests/lazyadam_ref.py and
// tests/rowwise_adagrad_ref.py.
// ------------------------------------------------------------------------------------------
template <int LPR, int NV, int OPT>
struct SparseOptApply {
    SideBufs rs, cs;
    SlotTwo s2;
    int d4, lg;
    OptConsts o;
    float inv_d;                        // 1 / d_model (RowWiseAdagrad's mean over the row's real columns)
    struct State { f4 A[NV], B[NV]; float Ab, Bb, Ar; };        // Ar: RowWiseAdagrad's one accumulator of the row
    __device__ void prefetch(bool is_row, int32_t id, State &st) const
    {
        const SideBufs &sb = is_row ? rs : cs;
        if (OPT == GLOVE_OPT_SGD && o.momentum == 0.f) return;
        if constexpr (OptSlots<OPT>::row_wise) {
            st.Ar = sb.S1[id];          // one float per id: no slot row is read
            st.Ab = sb.S1b[id];
            return;
        }
        load_row<LPR, NV>(st.A, sb.S1, id, d4, lg);
        st.Ab = sb.S1b[id];
        if (OptSlots<OPT>::two) {
            load_row<LPR, NV>(st.B, is_row ? s2.R : s2.C, id, d4, lg);
            st.Bb = (is_row ? s2.br : s2.bc)[id];
        }
    }
    __device__ void finish(bool is_row, int32_t id, int32_t wid, int q, f4 (&G)[NV], f4 (&Wv)[NV], float Gb, float bval, State &st) const
    {
        const SideBufs &sb = is_row ? rs : cs;
        const bool slots = !(OPT == GLOVE_OPT_SGD && o.momentum == 0.f);
        if constexpr (OptSlots<OPT>::row_wise) {
            // G is the id's finished sum here on both paths of for_each_id (a heavy id: group 0 has added the groups' partial
            // sums and the activity-L2 term before it calls): the square is of the sum, never a sum of partial squares
            rowwise_adagrad_row<LPR, NV>(Wv, st.Ar, G, o.lr, o.eps, inv_d);
            store_row<LPR, NV>(sb.W, (size_t)wid, d4, lg, Wv);
            if (lg == 0) {
                OptElem<OPT>::one(bval, st.Ab, st.Bb, Gb, o);
                sb.S1[id] = st.Ar;
                sb.S1b[id] = st.Ab;
                sb.bias[wid] = bval;
            }
            return;
        }
#pragma unroll
        for (int kk = 0; kk < NV; ++kk) {
            float w[4] = {Wv[kk].x, Wv[kk].y, Wv[kk].z, Wv[kk].w}, a[4] = {st.A[kk].x, st.A[kk].y, st.A[kk].z, st.A[kk].w};
            float b[4] = {st.B[kk].x, st.B[kk].y, st.B[kk].z, st.B[kk].w};
            const float g[4] = {G[kk].x, G[kk].y, G[kk].z, G[kk].w};
#pragma unroll
            for (int i = 0; i < 4; ++i) OptElem<OPT>::one(w[i], a[i], b[i], g[i], o);
            Wv[kk] = f4{w[0], w[1], w[2], w[3]};
            st.A[kk] = f4{a[0], a[1], a[2], a[3]};
            st.B[kk] = f4{b[0], b[1], b[2], b[3]};
        }
        if (slots) store_row<LPR, NV>(sb.S1, (size_t)id, d4, lg, st.A);
        if (OptSlots<OPT>::two) store_row<LPR, NV>(is_row ? s2.R : s2.C, (size_t)id, d4, lg, st.B);
        store_row<LPR, NV>(sb.W, (size_t)wid, d4, lg, Wv);
        if (lg == 0) {
            OptElem<OPT>::one(bval, st.Ab, st.Bb, Gb, o);
            if (slots) sb.S1b[id] = st.Ab;
            if (OptSlots<OPT>::two) (is_row ? s2.br : s2.bc)[id] = st.Bb;
            sb.bias[wid] = bval;
        }
    }
};

template <int LPR, int NV, int OPT>
__global__ __launch_bounds__(kBlock) void apply_sparse_opt_kernel(
    IdWork wk, SideBufs rs, SideBufs cs, SlotTwo s2, int d4, StepConsts k, OptConsts o,
    double ln_beta1, double ln_beta2, const int64_t *__restrict__ step, float *__restrict__ scalars,
    const float *__restrict__ blockpart, int nblocks_rowpass, float *__restrict__ loss_out)
{
    // t = global_step after rowpass advanced it (Adamax: lr_t = lr / (1 - beta1^t); LazyAdam: Adam's lr_t, bias-corrected by the
    // global t whenever a row was last touched)
    if (OPT == GLOVE_OPT_ADAMAX) o.lr_t = o.lr / -expm1f((float)((double)(*step) * ln_beta1));
    if (OPT == GLOVE_OPT_LAZYADAM) o.lr_t = adam_lr_t(o.lr, ln_beta1, ln_beta2, *step);
    const bool scalar_duty = for_each_id<LPR, NV>(wk, rs, cs, d4, k,
                                                  SparseOptApply<LPR, NV, OPT>{rs, cs, s2, d4, (int)(threadIdx.x % LPR), o, k.inv_d});
    if (scalar_duty) {
        float tot[kPartials];
        sum_blockpart(blockpart, nblocks_rowpass, tot);
        if (threadIdx.x == 0)
            scalar_epilogue<true>(tot, k, scalars, scalars, [&](float &gn, float &a, float &b, float dg) { OptElem<OPT>::one(gn, a, b, dg, o); },
                                  loss_out);
    }
}

// Keras-legacy RMSprop over [R | C | br | bc], consuming (and zeroing) G_flat: every rms entry decays, entries with a gradient move
__global__ __launch_bounds__(kBlock) void dense_rmsprop_kernel(
    DenseSegs segs, StepConsts k, float rho, float *__restrict__ scalars, float *__restrict__ tail,
    float *__restrict__ loss_out, int do_scalars)
{
#pragma clang fp contract(off)
    const DenseSeg sg = segs.s[blockIdx.y];
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < sg.n; i += (int64_t)gridDim.x * kBlock) {
        const float gv = sg.G[i];
        const float a = rho * sg.S1[i] + (1.0f - rho) * gv * gv;
        sg.S1[i] = a;
        if (gv != 0.f) {
            sg.W[i] -= k.lr * gv / (sqrtf(a) + k.eps);
            sg.G[i] = 0.f;
        }
    }
    if (do_scalars && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        const float g = scalars[0];
        const float tot[kPartials] = {tail[1], tail[2], tail[3], tail[0]};
        float loss, L, reg;
        loss_from_partials(tot, k, g, loss, L, reg);
        const float dg = tail[0] + 2.0f * k.m * k.l2 * g;
        const float a = rho * scalars[1] + (1.0f - rho) * dg * dg;
        scalars[1] = a;
        scalars[0] = g - k.lr * dg / (sqrtf(a) + k.eps);
        if (loss_out) { loss_out[0] = loss; loss_out[1] = L; loss_out[2] = reg; loss_out[3] = tail[0]; }
        tail[0] = tail[1] = tail[2] = tail[3] = 0.f;
    }
}

// ------------------------------------------------------------------------------------------
// Keras-legacy Adam in ONE launch behind the passes (single GPU, batches that touch a minority of the rows:
// the reference's default, 1,024 pairs against a 10^4-row vocabulary).  The passes left mark[id] = 1 for
// every id of the batch (in the bias segments of G_flat, which is otherwise unused on this path).
//   * the leading workgroups are the sparse apply: per distinct id, sum of the chunk partials -> m, v, W
//     (same traversal and summation order as the Adagrad apply and the dense-gradient kernel);
//   * the remaining workgroups sweep ALL rows, one lane group per row: a marked row belongs to the apply part
//     (its mark is cleared, nothing else), an unmarked row takes the G = 0 update m *= b1, v *= b2,
//     W -= lr_t m / (sqrt(v) + eps) — Keras' sparse Adam decays every row of the table, a11.
// The two parts touch disjoint rows, so they run side by side; only a row's own sweep group reads or clears
// its mark.  Results are bit-identical to dense_grad + dense_adam; G_flat is all zero again afterwards.
// ------------------------------------------------------------------------------------------
// (OPT: GLOVE_OPT_ADAM, or GLOVE_OPT_NADAM — Keras-legacy Nadam on the same two-part kernel: the legacy optimizer's sparse path
// decays m and v over the whole variable like its Adam, but only the touched rows move)
template <int LPR, int NV, int OPT>
struct DecayApply {
    SideBufs rs, cs;
    SlotTwo s2;
    int d4, lg;
    float lr_t, b1, b2, eps;            // Adam
    NadamConsts nk;                     // Nadam
    struct State { f4 M[NV], V[NV]; float Mb, Vb; };
    __device__ void prefetch(bool is_row, int32_t id, State &st) const
    {
        const SideBufs &sb = is_row ? rs : cs;
        load_row<LPR, NV>(st.M, sb.S1, id, d4, lg);
        load_row<LPR, NV>(st.V, is_row ? s2.R : s2.C, id, d4, lg);
        st.Mb = sb.S1b[id];
        st.Vb = (is_row ? s2.br : s2.bc)[id];
    }
    __device__ void finish(bool is_row, int32_t id, int32_t wid, int q, f4 (&G)[NV], f4 (&Wv)[NV], float Gb, float bval, State &st) const
    {
        const SideBufs &sb = is_row ? rs : cs;
#pragma unroll
        for (int kk = 0; kk < NV; ++kk) {
            if constexpr (OPT == GLOVE_OPT_ADAM) {
                adam_vec(Wv[kk], st.M[kk], st.V[kk], G[kk], lr_t, b1, b2, eps);
            } else {
                float w[4] = {Wv[kk].x, Wv[kk].y, Wv[kk].z, Wv[kk].w}, m[4] = {st.M[kk].x, st.M[kk].y, st.M[kk].z, st.M[kk].w};
                float v[4] = {st.V[kk].x, st.V[kk].y, st.V[kk].z, st.V[kk].w};
                const float g[4] = {G[kk].x, G[kk].y, G[kk].z, G[kk].w};
#pragma unroll
                for (int i = 0; i < 4; ++i) nadam_elem(w[i], m[i], v[i], g[i], nk);
                Wv[kk] = f4{w[0], w[1], w[2], w[3]};
                st.M[kk] = f4{m[0], m[1], m[2], m[3]};
                st.V[kk] = f4{v[0], v[1], v[2], v[3]};
            }
        }
        store_row<LPR, NV>(sb.S1, (size_t)id, d4, lg, st.M);
        store_row<LPR, NV>(is_row ? s2.R : s2.C, (size_t)id, d4, lg, st.V);
        store_row<LPR, NV>(sb.W, (size_t)id, d4, lg, Wv);
        if (lg == 0) {
            if constexpr (OPT == GLOVE_OPT_ADAM) adam_elem(bval, st.Mb, st.Vb, Gb, lr_t, b1, b2, eps);
            else nadam_elem(bval, st.Mb, st.Vb, Gb, nk);
            sb.S1b[id] = st.Mb;
            (is_row ? s2.br : s2.bc)[id] = st.Vb;
            sb.bias[id] = bval;
        }
    }
};

template <int LPR, int NV, int OPT>
__global__ __launch_bounds__(kBlock) void adam_fused_kernel(
    IdWork wk, SideBufs rs, SideBufs cs, SlotTwo s2, int d4, StepConsts k,
    float b1, float b2, double ln_beta1, double ln_beta2, const int64_t *__restrict__ step,
    float *__restrict__ scalars, const float *__restrict__ blockpart, int nblocks_rowpass,
    float *__restrict__ mark_rows, float *__restrict__ mark_cols, int V_row, int V, int apply_blocks,
    float *__restrict__ loss_out)
{
    constexpr int GPB = kBlock / LPR;
    constexpr bool kAdam = OPT == GLOVE_OPT_ADAM;
    const int lg = threadIdx.x % LPR;
    const float lr_t = kAdam ? adam_lr_t(k.lr, ln_beta1, ln_beta2, *step) : 0.f;
    NadamConsts nk = {};
    if (!kAdam) nk = nadam_consts(k.lr, k.eps, b1, b2, ln_beta2, *step, scalars);
    if ((int)blockIdx.x >= apply_blocks) {
        // ---- sweep: a lane group per table row (R's rows first, then C's), kSweepRows rows in flight per group so
        // that the whole sweep is resident in one round next to the register-heavier apply part
        const int sb0 = blockIdx.x - apply_blocks, nsb = gridDim.x - apply_blocks;
        sweep_unowned<LPR, NV, OPT>(FloatMarks{mark_rows, mark_cols}, rs, cs, s2, V_row, d4, sb0 * GPB + (int)threadIdx.x / LPR, nsb * GPB,
                                    V_row + V, lr_t, b1, b2, 0.f, k.eps);
        return;
    }
    // ---- apply: the ids of the batch (for_each_id sees a grid of apply_blocks workgroups)
    const bool scalar_duty = for_each_id<LPR, NV>(wk, rs, cs, d4, k, DecayApply<LPR, NV, OPT>{rs, cs, s2, d4, lg, lr_t, b1, b2, k.eps, nk},
                                                  apply_blocks);
    if (scalar_duty) {
        float tot[kPartials];
        sum_blockpart(blockpart, nblocks_rowpass, tot);
        if (threadIdx.x == 0) {
            scalar_epilogue<true, kAdam>(tot, k, scalars, scalars, [&](float &gn, float &m, float &v, float dg) {
                if constexpr (kAdam) adam_elem(gn, m, v, dg, lr_t, b1, b2, k.eps);
                else nadam_elem(gn, m, v, dg, nk);
            }, loss_out);
            if (!kAdam) scalars[4 + (int)(*step & 1)] = nk.sched_new;      // the momentum cache (see nadam_consts)
        }
    }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
static int check_common(const glove_plan *p, const glove_tables *t, const glove_hyper *h, const void *ws)
{
    if (!p || !t || !h || !ws) return GLOVE_E_BADARG;
    if (p->B < 0 || p->cap_chunks < 0 || t->V <= 0 || t->d <= 0 || (t->d % 4) != 0) return GLOVE_E_BADARG;
    if (!p->counts || !t->R || !t->C || !t->br || !t->bc || !t->scalars || !t->step) return GLOVE_E_BADARG;
    if (p->B > 0 && (!p->r_chunk_id || !p->r_chunk_start || !p->r_uniq_slot ||
                     !p->heavy || p->heavy_chunks < 1 || !p->r_uniq_rec || !p->c_uniq_rec || !p->c_chunk_id || !p->c_chunk_start || !p->c_uniq_slot))
        return GLOVE_E_BADARG;
    // the pair fields: in arrays of the plan's own, or (a plan of a dealt epoch, glove_plan_build_sorted) in its chunk records only
    const bool own_pairs = p->r_partner && p->r_w && p->r_y && p->c_partner && p->c_w && p->c_y;
    if (p->B > 0 && !own_pairs && !(p->r_crec && p->c_crec)) return GLOVE_E_BADARG;
    const RowShape shape = pick_row_shape(t->d / 4);
    if (shape.lpr == 0 || pick_pass_shape(t->d / 4).lpr == 0 || p->chunk_cap <= 0) return GLOVE_E_BADARG;
    if ((uint64_t)t->V * (uint64_t)t->d * 4u >= (1ull << 32) || t->V_row < 0 || t->V_row > t->V) return GLOVE_E_BADARG;   // 32-bit row offsets
    if (t->R_ver && 2ull * (uint64_t)(t->V_row > 0 ? t->V_row : t->V) * (uint64_t)t->d * 4u >= (1ull << 32)) return GLOVE_E_BADARG;
    if ((t->R_tag != nullptr) != (t->C_tag != nullptr) || (t->R_tag && t->R_ver)) return GLOVE_E_BADARG;   // tags: both tables, not beside R_ver
    if (t->R_tag && 2ull * (uint64_t)t->V * (uint64_t)t->d * 4u >= (1ull << 32)) return GLOVE_E_BADARG;
    if (t->d_model < 0 || t->d_model > t->d) return GLOVE_E_BADARG;
    if (p->chunk_cap > kChunkMax) return GLOVE_E_BADARG;
    if (h->head != GLOVE_HEAD_REGRESSION && h->head != GLOVE_HEAD_LOGISTIC) return GLOVE_E_BADARG;
    return 0;
}

static inline int sides_of(const glove_hyper *h) { return (h->sides & 3) ? (h->sides & 3) : 3; }
static inline int v_row(const glove_tables *t) { return t->V_row > 0 ? t->V_row : t->V; }

struct GradLayout { int64_t G_R, G_br, G_C, G_bc, tail, total; };
static GradLayout grad_layout(int32_t Vr, int32_t V, int32_t d)
{
    GradLayout L;
    auto up4 = [](int64_t x) { return (x + 3) / 4 * 4; };
    L.G_R = 0;
    L.G_br = (int64_t)Vr * d;
    L.G_C = up4(L.G_br + Vr);
    L.G_bc = L.G_C + (int64_t)V * d;
    L.tail = up4(L.G_bc + V);
    L.total = L.tail + 8;
    return L;
}

static IdWork id_work(const glove_plan *p)
{
    IdWork w;
    w.counts = p->counts;
    w.nu_r_host = p->host_counts[1];
    w.nu_c_host = p->host_counts[3];
    w.n_heavy_host = p->host_counts[4];
    w.heavy = p->heavy;
    w.heavy_blocks = p->host_counts[4] >= 0 ? p->host_counts[4] : p->cap_heavy;
    w.heavy_chunks = p->heavy_chunks;
    w.sides = 3;
    w.pre_r = w.pre_c = kFuseNone;
    w.per = 1;
    w.gpb = 0;
    w.work = nullptr;
    w.flips = 0;
    return w;
}

// the grid of an apply launch (for_each_id): the heavy ids' workgroups, the light ids' lane groups, one workgroup of scalar duty
static inline int apply_blocks(const glove_plan *p, RowShape shape)
{
    return id_work(p).heavy_blocks + blocks_for(2 * (int64_t)p->cap_uniq, kBlock / shape.lpr) + 1;
}

static StepConsts make_consts(const glove_tables *t, const glove_hyper *h)
{
    StepConsts k;
    const float dm = (float)(t->d_model > 0 ? t->d_model : t->d);      // the reference's embedding size
    k.kappa = 2.0f * h->reg_mult * h->l2_reg / dm * h->inv_batch;
    k.kappa_b = 2.0f * h->reg_mult * h->l2_reg * h->inv_batch;
    k.lr = h->learning_rate;
    k.eps = h->epsilon;
    k.l2 = h->l2_reg;
    k.m = h->reg_mult;
    k.inv_batch = h->inv_batch;
    k.inv_d = 1.0f / dm;
    return k;
}

// Opens the call of an entry point: the arguments every step-path call shares are checked here, once, and nowhere behind it.
// `carved`: the workspace holds the layout of carve_step_ws and must have its size (the one-launch chains keep their own records
// there instead: launch_tagged_chain)
static int open_call(StepCall &c, const glove_plan *p, const glove_tables *t, const glove_hyper *h, void *ws, size_t ws_bytes,
                     void *stream, bool carved = true)
{
    if (int rc = check_common(p, t, h, ws)) return rc;
    const int d4 = t->d / 4;
    c = StepCall{p, t, h, ws, ws_bytes, (hipStream_t)stream, carve_step_ws(ws, p->B, p->cap_chunks, t->d), d4, pick_row_shape(d4),
                 pick_pass_shape(d4), sides_of(h), make_consts(t, h)};
    return carved && c.w.bytes > ws_bytes ? GLOVE_E_WORKSPACE : 0;
}

// The optimizer's own hyper-parameters as the apply kernels take them; the logs of the betas in fp64 (adam_lr_t)
struct OptHyper { OptConsts o; float b1, b2; double ln_b1, ln_b2; };
static OptHyper opt_consts(const glove_hyper *h)
{
    OptHyper x;
    x.b1 = (float)h->beta1;
    x.b2 = (float)h->beta2;
    x.o = {h->learning_rate, h->epsilon, h->momentum, 0.f, x.b1, x.b2, h->nesterov ? 1 : 0, h->rho};
    // (an optimizer without betas leaves them unchecked, and its kernels do not read the logs: 0 then, as for a beta out of range)
    x.ln_b1 = x.b1 > 0.f ? log((double)x.b1) : 0.0;
    x.ln_b2 = x.b2 > 0.f ? log((double)x.b2) : 0.0;
    return x;
}

// Optimizer `opt` (glove_hyper.optimizer, or the one an entry point stands for) on `sides` (1 rows, 2 cols, 3 both): its slots are
// there and its hyper-parameters are in range
static int check_optimizer(const glove_tables *t, const glove_hyper *h, int sides, int opt)
{
    const bool betas = opt == GLOVE_OPT_ADAMAX || opt == GLOVE_OPT_NADAM || opt == GLOVE_OPT_ADAM || opt == GLOVE_OPT_LAZYADAM;
    const bool two_slots = betas || opt == GLOVE_OPT_ADADELTA || opt == GLOVE_OPT_FTRL;
    // (RowWiseAdagrad: one slot — s1_R / s1_C are float[rows] —, no hyper-parameter of its own beside Adagrad's epsilon)
    if (opt != GLOVE_OPT_ADAGRAD && opt != GLOVE_OPT_SGD && opt != GLOVE_OPT_RMSPROP && opt != GLOVE_OPT_ROWWISE_ADAGRAD && !two_slots)
        return GLOVE_E_BADARG;
    if ((sides & 1) && (!t->s1_R || !t->s1_br || (two_slots && (!t->s2_R || !t->s2_br)))) return GLOVE_E_BADARG;
    if ((sides & 2) && (!t->s1_C || !t->s1_bc || (two_slots && (!t->s2_C || !t->s2_bc)))) return GLOVE_E_BADARG;
    if (betas && (!(h->beta1 > 0.0 && h->beta1 < 1.0) || !(h->beta2 > 0.0 && h->beta2 < 1.0) || !t->step)) return GLOVE_E_BADARG;
    if ((opt == GLOVE_OPT_ADADELTA || opt == GLOVE_OPT_RMSPROP) && !(h->rho > 0.f && h->rho < 1.f)) return GLOVE_E_BADARG;
    if (opt == GLOVE_OPT_FTRL && !(h->learning_rate > 0.f)) return GLOVE_E_BADARG;
    if (opt == GLOVE_OPT_SGD && !(h->momentum >= 0.f && h->momentum < 1.f)) return GLOVE_E_BADARG;
    return 0;
}

// A run-time optimizer as the compile-time OPT of a launch: f(std::integral_constant<int, OPT>) for the one of OPTS that opt is
template <int... OPTS, class F>
static bool dispatch_opt(int opt, F f)
{
    return ((opt == OPTS ? (f(std::integral_constant<int, OPTS>{}), true) : false) || ...);
}
static inline int rowpass_blocks(const glove_plan *p, int lpr) { return blocks_for(p->cap_chunks, kBlock / lpr); }

// FUSE passes: consecutive chunks per lane group.  Up to 6 (12 until round 5, see below): a heavy id then leaves one partial row per 12 chunks instead
// of one per chunk, and an id of a few chunks is usually applied by the pass itself (an id whose chunks straddle two
// groups goes through partial rows and the apply launch) — but the ids of the Zipf head fill consecutive FULL chunks, so
// a head group's per x chunk_cap pairs are one serial chain of partner-row trips, the launch's critical path once per is
// large.  One-process A/B of the whole step on resident plans, B = 1 M, chunk_cap 32 (tools/ab_kernels.py, builds with
// a forced per): V = 400 k, d = 300: per 4 / 8 / 12 / 16 / 20 / 23 / 27 / 32 / 48 = 620 / 613 / 609 / 640 / 699 / 772 /
// 868 / 979 / 1281 us; V = 2 M, d = 128: 516 / 509 / 520 / 536 / 541 / 572 / - / 565 / 765 (builds differ by +-1.5 % whatever
// they hold: 12 and the former rule's 12 / 18 are not told apart).  Fewer when the side has too few
// chunks to fill the chip with such groups (V = 400 k at B = 131,072: per 1 or 2 156 us, per 4 165 us; V = 50 k: 103 /
// 103 / 106), more only when the plan has more chunks than kMaxPassBlocks workgroups of such groups cover (the loss
// partials are kept per workgroup).
// Solid workgroups (sidepass_kernel, Slots) pay where the head of the batch leaves hundreds of partial rows: from 131,072 chunks a
// side (V = 400 k, d = 300, one process, same plans: B = 1 M 565.3 -> 557.7 us per step; at B = 131,072 — 50 k chunks, the id of
// rank 1 in 50 runs — the head workgroups' epilogue is on the passes' critical path: 139.3 -> 142.4).  Pass and apply launch ask here.
static bool solid_groups(const glove_plan *p)
{
    const int64_t r = most_chunks(p, true), c = most_chunks(p, false);
    return (r > c ? r : c) >= 131072;
}

static int fuse_per(const glove_plan *p, int lpr)
{
    const int64_t nr = most_chunks(p, true), nc = most_chunks(p, false);
    const int64_t side = nr > nc ? nr : nc;
    int per = (int)((side + 16383) / 16384);              // <= 2,048 workgroups up to 196 k chunks a side
    // (round 5, the passes compiled for one head with staged version lookups — shorter per-chunk chains, more waves: the same
    // A/B, one process, us per step: V = 400 k, d = 300: per 3 / 4 / 5 / 6 / 8 / 10 / 12 / 15 = 558 / 546 / 543 / 540 / 545* / 551* / 550 / 595*;
    // V = 2 M, d = 128: 344.6 / 344.5 / 344.4 / 343.1 / 344* / 348* / 348.5 / 431* (* scaled from another box's run against 12): 6)
    per = per < 1 ? 1 : per > 6 ? 6 : per;
    const int64_t groups = (int64_t)kMaxPassBlocks * (kBlock / lpr);
    // (`side` is the chunk count itself when the host knows it — also for a staging plan whose counts were read back: its
    // capacity is the worst case, V = 2 M at B = 1 M ran 16 chunks per group instead of 12 for nothing, 530 against 511 us)
    const int need = (int)((side + groups - 1) / groups);
    return need > per ? need : per;
}
static inline int fusepass_blocks(const glove_plan *p, int lpr, int per, bool row)
{
    const int64_t per_block = (int64_t)per * (kBlock / lpr);
    const int64_t b = (most_chunks(p, row) + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : b > kMaxPassBlocks ? kMaxPassBlocks : b);
}

static SideBufs side_bufs(const glove_plan *p, const StepWs &w, const glove_tables *t, bool row)
{
    SideBufs s;
    s.uniq_rec = row ? p->r_uniq_rec : p->c_uniq_rec;
    s.gp = row ? w.gp_r : w.gp_c;
    s.gb = row ? w.gb_r : w.gb_c;
    s.W = row ? t->R : t->C;
    s.S1 = row ? t->s1_R : t->s1_C;
    s.bias = row ? t->br : t->bc;
    s.S1b = row ? t->s1_br : t->s1_bc;
    s.ver = nullptr;            // set by the twin step alone: every other caller sees a canonical table
    s.twin = 0;
    return s;
}

// What a launch over the batch's ids (for_each_id) takes: the ids of `sides`, behind passes that fused pre_r / pre_c (the twin
// step's caller has seen R_ver); the grid, and the workgroups of the row-side pass whose loss partials the scalar duty sums
struct IdLaunch { IdWork wk; SideBufs rs, cs; int nb, nb_row; };
static IdLaunch id_launch(const StepCall &c, int sides, int pre_r = kFuseNone, int pre_c = kFuseNone)
{
    IdLaunch l{id_work(c.p), side_bufs(c.p, c.w, c.t, true), side_bufs(c.p, c.w, c.t, false), apply_blocks(c.p, c.shape), 0};
    const bool fused = pre_r != kFuseNone || pre_c != kFuseNone, pack = pre_r == kFusePack || pre_c == kFusePack;
    l.wk.sides = sides;
    l.wk.pre_r = pre_r;
    l.wk.pre_c = pre_c;
    l.wk.per = fused ? fuse_per(c.p, c.pass.lpr) : 1;
    l.wk.gpb = fused && !pack && solid_groups(c.p) ? kBlock / c.pass.lpr : 0;      // (as launch_passes: the packing passes are never solid)
    // (the first launch of the step; behind the packing row pass its grid too — or folded by glove_rowside_step_adagrad_f32: any count reads them)
    l.nb_row = fused ? fusepass_blocks(c.p, c.pass.lpr, l.wk.per, true) : rowpass_blocks(c.p, c.pass.lpr);
    if (pre_r == kFuseTwin) {
        l.rs.ver = c.t->R_ver;
        l.rs.twin = v_row(c.t);
    }
    return l;
}

// One side of a one-launch step: S = OneSide (Adagrad: the step tags) or AdamSide (the second slot, the bitmap of the batch's ids)
template <class S>
static S step_side(const glove_plan *p, const glove_tables *t, bool row)
{
    S s;
    s.crec = row ? p->r_crec : p->c_crec;
    s.own = row ? t->R : t->C;
    s.own_bias = row ? t->br : t->bc;
    s.other = row ? t->C : t->R;
    s.other_bias = row ? t->bc : t->br;
    s.S1 = row ? t->s1_R : t->s1_C;
    s.S1b = row ? t->s1_br : t->s1_bc;
    if constexpr (std::is_same<S, AdamSide>::value) {
        s.S2 = row ? t->s2_R : t->s2_C;
        s.S2b = row ? t->s2_br : t->s2_bc;
        s.mark = row ? p->r_mark : p->c_mark;
    } else {
        s.own_tag = row ? t->R_tag : t->C_tag;
        s.other_tag = row ? t->C_tag : t->R_tag;
    }
    s.own_twin = row ? v_row(t) : t->V;
    s.other_twin = row ? t->V : v_row(t);
    s.n_host = p->host_counts[row ? 0 : 2];
    s.count_index = row ? 0 : 2;
    s.capP = rec_cap(p->chunk_cap);
    s.cap_chunks = p->cap_chunks > 0 ? p->cap_chunks : 1;
    return s;
}

static inline SlotTwo slot_two(const glove_tables *t) { return SlotTwo{t->s2_R, t->s2_C, t->s2_br, t->s2_bc}; }

#ifdef GLOVE_STAMPS
GLOVE_STAMPS_SETTER(set_stamps_step)
#endif

}  // namespace glove

using namespace glove;

extern "C" {

int glove_abi_version(void) { return GLOVE_ABI_VERSION; }

// Every entry point but the twin form of the Adagrad step reads and writes rows 0 .. V_row-1 of a twinned row table: it first
// brings the table back to that form (one small launch over V_row version bytes plus the rows whose second copy was
// current; nothing without a twin).  A caller that mixes step forms, or steps and anything else, on one twinned table
// therefore never reads a stale copy.
static int plain_table(const glove_tables *t, void *stream) { return t && (t->R_ver || t->R_tag) ? glove_canonicalize_f32(t, stream) : 0; }
#ifdef GLOVE_STAMPS
int glove_debug_set_stamps(void *p)
{
    // every object whose kernels stamp holds a g_stamps of its own (glove_common.h)
    for (auto set : {set_stamps_step, set_stamps_passes_lpr8, set_stamps_passes_mid, set_stamps_passes_wide})
        if (int rc = set(p)) return rc;
    return 0;
}
#endif

size_t glove_step_workspace_bytes(int64_t B, int32_t cap_chunks, int32_t d)
{
    if (B < 0 || cap_chunks < 0 || d <= 0) return 0;
    return carve_step_ws(nullptr, B, cap_chunks, d).bytes;
}


size_t glove_dense_grad_layout(int32_t V_row, int32_t V, int32_t d, int64_t *offs)
{
    const GradLayout L = grad_layout(V_row > 0 ? V_row : V, V, d);
    if (offs) { offs[0] = L.G_R; offs[1] = L.G_br; offs[2] = L.G_C; offs[3] = L.G_bc; offs[4] = L.tail; }
    return (size_t)L.total;
}

static PassSide pass_side(const glove_plan *p, const glove_tables *t, const StepWs &w, bool row, bool want_e = false,
                          int fuse = kFuseNone, bool twin = false)
{
    PassSide sd;
    sd.partner = row ? p->r_partner : p->c_partner;
    sd.w = row ? p->r_w : p->c_w;
    sd.y = row ? p->r_y : p->c_y;
    sd.chunk_id = row ? p->r_chunk_id : p->c_chunk_id;
    sd.chunk_start = row ? p->r_chunk_start : p->c_chunk_start;
    sd.own = row ? t->R : t->C;
    sd.other = row ? t->C : t->R;
    sd.own_bias = row ? t->br : t->bc;
    sd.other_bias = row ? t->bc : t->br;
    sd.gp = row ? w.gp_r : w.gp_c;
    sd.gb = row ? w.gb_r : w.gb_c;
    sd.e_out = row && want_e ? w.e : nullptr;
    sd.mark = nullptr;
    sd.n_host = p->host_counts[row ? 0 : 2];
    sd.count_index = row ? 0 : 2;
    sd.crec = row ? p->r_crec : p->c_crec;
    sd.chunk_hw = row ? p->r_chunk_hw : p->c_chunk_hw;
    sd.capP = rec_cap(p->chunk_cap);
    sd.fuse = fuse;
    sd.own_out = row ? t->R : t->C;
    sd.own_bias_out = row ? t->br : t->bc;
    sd.S1 = row ? t->s1_R : t->s1_C;
    sd.S1b = row ? t->s1_br : t->s1_bc;
    // the row table is the one that may be twinned: own of the row side, partner of the col side
    sd.own_ver = twin && row ? t->R_ver : nullptr;
    sd.other_ver = twin && !row ? t->R_ver : nullptr;
    sd.own_twin = sd.other_twin = v_row(t);
    return sd;
}

static inline bool has_slot1(const glove_tables *t) { return t->s1_R && t->s1_C && t->s1_br && t->s1_bc; }

// What a launch of the passes does beyond the plain pass of its sides; a call site names only that
struct PassOpts {
    int which;                                          // 1 = row side, 2 = col side, 3 = both in one launch
    float *mark_rows = nullptr, *mark_cols = nullptr;   // the batch's ids marked (the Adam steps' sweeps leave those rows alone)
    bool want_e = false;                                // the diagnostic row pass: e by pair position
    int fuse_r = kFuseNone, fuse_c = kFuseNone;
    bool twin = false;                                  // follow the version bytes of a twinned row table
    float *packed = nullptr;                            // the list kFusePack writes
    bool list_tail = false;                             // the twin form's col-side launch lists the apply launch's ids
    explicit PassOpts(int which_) : which(which_) {}
    PassOpts &marks(float *rows, float *cols) { mark_rows = rows; mark_cols = cols; return *this; }
    PassOpts &with_e() { want_e = true; return *this; }
    PassOpts &fuse(int r, int c) { fuse_r = r; fuse_c = c; return *this; }
    PassOpts &on_twin(bool tail = false) { twin = true; list_tail = tail; return *this; }
    PassOpts &packing(float *list) { packed = list; return fuse(which & 1 ? kFusePack : kFuseNone, which & 2 ? kFusePack : kFuseNone); }
    bool packs() const { return fuse_r == kFusePack || fuse_c == kFusePack; }
    // (the diagnostic row pass stores e by pair position, which the records do not carry: it reads the plain arrays)
    bool records(const glove_plan *p) const { return p->r_crec != nullptr && p->c_crec != nullptr && !want_e; }
};

// Everything a launch of the passes can refuse, launch_passes' first act: an entry point asks before its own first launch
static int check_passes(const StepCall &c, const PassOpts &o)
{
    const glove_plan *p = c.p;
    const glove_tables *t = c.t;
    if ((o.twin || o.fuse_r == kFuseTwin) && !t->R_ver) return GLOVE_E_BADARG;
    if (o.fuse_c == kFuseTwin) return GLOVE_E_BADARG;          // only the row table has a twin
    const bool applies = o.twin || (o.fuse_r != kFuseNone && o.fuse_r != kFusePack) || (o.fuse_c != kFuseNone && o.fuse_c != kFusePack);
    if (applies && !has_slot1(t)) return GLOVE_E_BADARG;
    // in place is only legal for a side whose table no concurrent chunk gathers from: one side per launch
    if ((o.fuse_r == kFuseInPlace && (o.which & 2)) || (o.fuse_c == kFuseInPlace && (o.which & 1))) return GLOVE_E_BADARG;
    // the packing build neither applies nor reads plain arrays: records, and no other fuse mode beside it
    if (o.packs() && (!o.packed || p->host_counts[1] < 0 || !p->r_crec || !p->c_crec || o.want_e || applies)) return GLOVE_E_BADARG;
    if (o.list_tail && (!o.twin || o.which != 2 || o.fuse_c != kFuseInPlace || !c.w.work || c.sides != 3)) return GLOVE_E_BADARG;
    if (!o.records(p) && p->B > 0 && !p->r_partner) return GLOVE_E_BADARG;     // (the diagnostic pass needs pair arrays)
    return 0;
}

static int launch_passes(const StepCall &c, const PassOpts &o)
{
    if (int rc = check_passes(c, o)) return rc;
    const glove_plan *p = c.p;
    const glove_tables *t = c.t;
    const RowShape shape = c.pass;
    const int which = o.which, fuse_r = o.fuse_r, fuse_c = o.fuse_c;
    const bool twin = o.twin, pack = o.packs(), fuse = fuse_r != kFuseNone || fuse_c != kFuseNone || twin;
    const int per = fuse ? fuse_per(p, shape.lpr) : 1;
    const int row_blocks = !(which & 1) ? 0 : fuse ? fusepass_blocks(p, shape.lpr, per, true) : rowpass_blocks(p, shape.lpr);
    const int nb = row_blocks + (!(which & 2) ? 0 : fuse ? fusepass_blocks(p, shape.lpr, per, false) : rowpass_blocks(p, shape.lpr));
    PassSide rs = pass_side(p, t, c.w, true, o.want_e, fuse_r, twin), cs = pass_side(p, t, c.w, false, false, fuse_c, twin);
    rs.mark = o.mark_rows;
    cs.mark = o.mark_cols;
    if (pack) {
        rs.own_out = cs.own_out = o.packed;
        rs.own_twin = 1;                                                  // behind the header
        cs.own_twin = 1 + (fuse_r == kFusePack ? p->host_counts[1] : 0);  // and behind the row side's ids when both sides pack
    }
    // the twin form's col-side launch: behind the pass, the workgroups that list the ids the apply launch has to visit
    ListTail tail{p->counts, p->r_uniq_rec, p->c_uniq_rec, p->host_counts[1], p->host_counts[3], p->heavy_chunks, per, -1};
    int nb_launch = nb;
    if (o.list_tail) {
        const int64_t ids = tail.nu_r_host >= 0 && tail.nu_c_host >= 0 ? (int64_t)tail.nu_r_host + tail.nu_c_host : 2 * (int64_t)p->cap_uniq;
        tail.first_block = nb;
        nb_launch = nb + (int)((ids + kBlock - 1) / kBlock);
    }
    const bool solid = fuse && !pack && solid_groups(p);        // (the applying run-merged passes: FUSE == 1)
    // the twin form's streaming cache policy: row tables beyond the Infinity Cache's reach (on the 61 MB table of V = 50 k, d = 300
    // it costs 3 - 8 %: the next launch finds the finished rows in the caches there)
    const bool streaming = (size_t)v_row(t) * (size_t)t->d * 4 >= ((size_t)128 << 20);
    // sidepass_kernel's builds live in four objects, by shape.  The wide shapes of one float4 per lane stay here: their code is the
    // one-unit build's only in a module that also holds the per-id apply functors (profiles/r11_step_units_resource_usage.txt)
    const PassLaunch a{c, rs, cs, tail, per, row_blocks, nb, nb_launch, which, twin, solid, streaming, o.records(p), pack, fuse};
    int rc;
    if (shape.lpr == 8) rc = launch_passes_lpr8(a);                                 // <8, 1>, <8, 2>
    else if (shape.nv == 1) rc = launch_pass_shapes<32, 1, 64, 1>(a);
    else if (shape.lpr * shape.nv <= 128) rc = launch_passes_mid(a);                // <32, 3>, <64, 2>
    else rc = launch_passes_wide(a);                                                // <64, 3>, <64, 4>
    if (rc) return rc;
    return (int)hipGetLastError();
}

// One launch of the passes as an entry point: refused before anything is launched, a twinned table brought home first
static int passes_on_plain_table(const StepCall &c, const PassOpts &o)
{
    if (int rc = check_passes(c, o)) return rc;
    if (int rc = plain_table(c.t, c.st)) return rc;
    return launch_passes(c, o);
}

int glove_passes_f32(const glove_plan *p, const glove_tables *t, const glove_hyper *h, void *ws, size_t ws_bytes,
                     void *stream)
{
    StepCall c;
    if (int rc = open_call(c, p, t, h, ws, ws_bytes, stream)) return rc;
    return passes_on_plain_table(c, PassOpts(3));
}

int glove_rowpass_f32(const glove_plan *p, const glove_tables *t, const glove_hyper *h, void *ws, size_t ws_bytes,
                      void *stream)
{
    StepCall c;
    if (int rc = open_call(c, p, t, h, ws, ws_bytes, stream)) return rc;
    return passes_on_plain_table(c, PassOpts(1).with_e());
}

int glove_colpass_f32(const glove_plan *p, const glove_tables *t, const glove_hyper *h, void *ws, size_t ws_bytes,
                      void *stream)
{
    StepCall c;
    if (int rc = open_call(c, p, t, h, ws, ws_bytes, stream)) return rc;
    return passes_on_plain_table(c, PassOpts(2));
}

// (its caller has seen the Adagrad slots — has_slot1 —, and R_ver where pre_r is kFuseTwin)
static int launch_apply_adagrad(const StepCall &c, float *loss_out, int pre_r, int pre_c, bool listed = false)
{
    IdLaunch l = id_launch(c, c.sides, pre_r, pre_c);
    IdWork &wk = l.wk;
    int32_t *const work = c.w.work;
    const bool short_list = (pre_r == kFuseTwin && pre_c == kFuseInPlace && wk.sides == 3) ||
                            (pre_r == kFuseInPlace && wk.sides == 1);        // glove_rowside_step_adagrad_f32
    if (listed) {
        // the col-side launch drew the list (ListTail); the finished row ids' version flips are this launch's (for_each_id)
        if (!(pre_r == kFuseTwin && pre_c == kFuseInPlace && wk.sides == 3) || !work) return GLOVE_E_BADARG;
        wk.work = work;
        wk.flips = 1;
    } else if (short_list && work) {
        // sort the ids out first (triage_kernel, a thread per id): the launch below then walks the list of those that
        // still need it.  Only where that list is short — the twin form, whose finished ids need a version flip at most
        // (V = 400 k, d = 300: apply 62 -> 12 us + 5 us of triage), and the in-place row side of the sharded forms,
        // whose finished ids need nothing.  Behind the slot form every row id still needs its
        // copy, nearly all ids go onto the list and its one counter becomes the bottleneck (V = 2 M: 51 us of triage)
        wk.work = work;
        // (a plan refilled on the device: a thread per id the arrays can hold, the kernel reads the counts)
        const int64_t ids = wk.nu_r_host >= 0 && wk.nu_c_host >= 0 ? (int64_t)wk.nu_r_host + wk.nu_c_host : 2 * (int64_t)c.p->cap_uniq;
        const int nbt = (int)((ids + kBlock - 1) / kBlock);
        if (nbt > 0) hipLaunchKernelGGL(triage_kernel, dim3(nbt), dim3(kBlock), 0, c.st, wk, l.rs, l.cs, work);
    }
#define CALL(LPR, NV)                                                                                             \
    hipLaunchKernelGGL((apply_adagrad_kernel<LPR, NV>), dim3(l.nb), dim3(kBlock), 0, c.st, wk, l.rs, l.cs, c.d4, \
                       c.k, c.t->scalars, c.w.blockpart, l.nb_row, loss_out)
    GLOVE_DISPATCH_ROW_SHAPE(c.shape, CALL);
#undef CALL
    return (int)hipGetLastError();
}

int glove_apply_adagrad_f32(const glove_plan *p, const glove_tables *t, const glove_hyper *h, void *ws,
                            size_t ws_bytes, float *loss_out, void *stream)
{
    StepCall c;
    if (int rc = open_call(c, p, t, h, ws, ws_bytes, stream)) return rc;
    if (!has_slot1(t)) return GLOVE_E_BADARG;
    if (int rc = plain_table(t, stream)) return rc;
    return launch_apply_adagrad(c, loss_out, kFuseNone, kFuseNone);
}

// (its caller has seen G_flat)
static int launch_dense_grad(const StepCall &c, float *G_flat)
{
    const IdLaunch l = id_launch(c, c.sides);
    const GradLayout L = grad_layout(v_row(c.t), c.t->V, c.t->d);
    float *G_R = G_flat + L.G_R, *G_C = G_flat + L.G_C, *G_br = G_flat + L.G_br, *G_bc = G_flat + L.G_bc,
          *tail = G_flat + L.tail;
#define CALL(LPR, NV)                                                                                                  \
    hipLaunchKernelGGL((dense_grad_kernel<LPR, NV>), dim3(l.nb), dim3(kBlock), 0, c.st, l.wk, l.rs, l.cs, c.d4,       \
                       c.k, G_R, G_C, G_br, G_bc, tail, c.w.blockpart, l.nb_row)
    GLOVE_DISPATCH_ROW_SHAPE(c.shape, CALL);
#undef CALL
    return (int)hipGetLastError();
}

int glove_dense_grad_f32(const glove_plan *p, const glove_tables *t, const glove_hyper *h, void *ws, size_t ws_bytes,
                         float *G_flat, void *stream)
{
    StepCall c;
    if (int rc = open_call(c, p, t, h, ws, ws_bytes, stream)) return rc;
    if (!G_flat) return GLOVE_E_BADARG;
    if (int rc = plain_table(t, stream)) return rc;
    return launch_dense_grad(c, G_flat);
}

// A dense sweep's launch: the four segments of the tables and of G_flat, the grid, whether the scalar work is its own
struct DenseSweep { DenseSegs segs; float *tail; int nbx, do_scalars; };

static int dense_common(const glove_tables *t, const glove_hyper *h, float *G_flat, bool adam, DenseSweep &sw)
{
    DenseSegs &segs = sw.segs;
    if (!t || !h || !G_flat || t->V <= 0 || t->d <= 0 || (t->d % 4) != 0 || t->d_model < 0 || t->d_model > t->d)
        return GLOVE_E_BADARG;
    if (!t->R || !t->C || !t->br || !t->bc || !t->scalars || !t->step) return GLOVE_E_BADARG;
    if (!t->s1_R || !t->s1_C || !t->s1_br || !t->s1_bc) return GLOVE_E_BADARG;
    if (adam && (!t->s2_R || !t->s2_C || !t->s2_br || !t->s2_bc)) return GLOVE_E_BADARG;
    const int32_t Vr = v_row(t);
    const GradLayout L = grad_layout(Vr, t->V, t->d);
    sw.tail = G_flat + L.tail;
    const int sides = sides_of(h);
    sw.do_scalars = (sides & 2) ? 1 : 0;
    // segment order = grid.y: 0 R, 1 C (float4 bodies), 2 br, 3 bc (scalar); a side that is not covered gets n = 0
    const int64_t nr = (sides & 1) ? 1 : 0, nc = (sides & 2) ? 1 : 0;
    segs.s[0] = {t->R, t->s1_R, t->s2_R, G_flat + L.G_R, nr * Vr * t->d};
    segs.s[1] = {t->C, t->s1_C, t->s2_C, G_flat + L.G_C, nc * t->V * t->d};
    segs.s[2] = {t->br, t->s1_br, t->s2_br, G_flat + L.G_br, nr * Vr};
    segs.s[3] = {t->bc, t->s1_bc, t->s2_bc, G_flat + L.G_bc, nc * t->V};
    sw.nbx = blocks_for((int64_t)(Vr > t->V ? Vr : t->V) * t->d / 4, kBlock);
    return 0;
}

int glove_dense_adagrad_f32(const glove_tables *t, const glove_hyper *h, float *G_flat, float *loss_out, void *stream)
{
    DenseSweep sw;
    if (h && h->optimizer == GLOVE_OPT_ROWWISE_ADAGRAD) return GLOVE_E_BADARG;      // its table slots are float[rows]: nothing to sweep
    if (int rc = dense_common(t, h, G_flat, false, sw)) return rc;
    if (int rc = plain_table(t, stream)) return rc;
    hipLaunchKernelGGL(dense_adagrad_kernel, dim3(sw.nbx, 4), dim3(kBlock), 0, (hipStream_t)stream, sw.segs, make_consts(t, h), t->scalars,
                       sw.tail, loss_out, sw.do_scalars);
    return (int)hipGetLastError();
}

// The dense sweep of glove_hyper.optimizer over G_flat: Adam's, or RMSprop's — the other dense-decay optimizer of the Keras set:
// its whole rms slot decays every step, entries with a gradient move.  What it refuses, and its launch.
static int check_dense_sweep(const glove_tables *t, const glove_hyper *h, float *G_flat, DenseSweep &sw)
{
    // touched rows only: no dense sweep (RowWiseAdagrad's table slots are not even shaped like the tables a sweep walks)
    if (h && (h->optimizer == GLOVE_OPT_LAZYADAM || h->optimizer == GLOVE_OPT_ROWWISE_ADAGRAD)) return GLOVE_E_BADARG;
    const bool rmsprop = h && h->optimizer == GLOVE_OPT_RMSPROP;
    if (int rc = dense_common(t, h, G_flat, !rmsprop, sw)) return rc;
    if (rmsprop) return h->rho > 0.f && h->rho < 1.f ? 0 : GLOVE_E_BADARG;
    return h->beta1 > 0.0 && h->beta1 < 1.0 && h->beta2 > 0.0 && h->beta2 < 1.0 ? 0 : GLOVE_E_BADARG;
}

static int launch_dense_sweep(const glove_tables *t, const glove_hyper *h, const DenseSweep &sw, float *loss_out, hipStream_t st)
{
    const StepConsts k = make_consts(t, h);
    if (h->optimizer == GLOVE_OPT_RMSPROP)
        hipLaunchKernelGGL(dense_rmsprop_kernel, dim3(sw.nbx, 4), dim3(kBlock), 0, st, sw.segs, k, h->rho, t->scalars, sw.tail, loss_out,
                           sw.do_scalars);
    else
        hipLaunchKernelGGL(dense_adam_kernel, dim3(sw.nbx, 4), dim3(kBlock), 0, st, sw.segs, k, (float)h->beta1, (float)h->beta2,
                           log((double)(float)h->beta1), log((double)(float)h->beta2), t->step, t->scalars, sw.tail, loss_out, sw.do_scalars);
    return (int)hipGetLastError();
}

// (on a G_flat that holds the ranks' summed gradients: the data-parallel step)
int glove_dense_adam_f32(const glove_tables *t, const glove_hyper *h, float *G_flat, float *loss_out, void *stream)
{
    DenseSweep sw;
    if (int rc = check_dense_sweep(t, h, G_flat, sw)) return rc;
    if (int rc = plain_table(t, stream)) return rc;
    return launch_dense_sweep(t, h, sw, loss_out, (hipStream_t)stream);
}

// The passes of `which`, their summed gradients into G_flat, the dense sweep over it: refused as a whole before the first launch
static int dense_step(const StepCall &c, int which, float *G_flat, float *loss_out)
{
    DenseSweep sw;
    if (int rc = check_dense_sweep(c.t, c.h, G_flat, sw)) return rc;
    if (int rc = plain_table(c.t, c.st)) return rc;
    if (int rc = launch_passes(c, PassOpts(which))) return rc;
    if (int rc = launch_dense_grad(c, G_flat)) return rc;
    return launch_dense_sweep(c.t, c.h, sw, loss_out, c.st);
}

static_assert(GLOVE_PACKED_ENTRY_FLOATS(0) == (size_t)kPackExtra, "the header's entry size is the kernels'");

// The passes can write packed-list entries themselves when the plan has chunk records (run-merged schedule) and its
// counts are known on the host (the col side's entries start behind the row side's).
static bool packing_ok(const glove_plan *p)
{
    return p->r_crec && p->c_crec && p->host_counts[1] >= 0 && p->host_counts[3] >= 0;
}

// header + every distinct id of the selected sides must fit (the plan's capacity bounds the counts not yet known here)
static bool packed_fits(const StepCall &c, int64_t capacity_entries)
{
    const glove_plan *p = c.p;
    const int64_t nr = (c.sides & 1) ? (p->host_counts[1] >= 0 ? p->host_counts[1] : p->cap_uniq) : 0;
    const int64_t nc = (c.sides & 2) ? (p->host_counts[3] >= 0 ? p->host_counts[3] : p->cap_uniq) : 0;
    return 1 + nr + nc <= capacity_entries;
}

// The batch's gradients as a packed list: of every id, or (`rest`, where the plan let glove_passes_packing_f32's passes pack) of
// the ids those passes left
static int pack_ids(const glove_plan *p, const glove_tables *t, const glove_hyper *h, void *ws, size_t ws_bytes, float *packed,
                    int64_t capacity_entries, void *stream, bool rest)
{
    StepCall c;
    if (int rc = open_call(c, p, t, h, ws, ws_bytes, stream)) return rc;
    if (!packed) return GLOVE_E_BADARG;
    if (!packed_fits(c, capacity_entries)) return GLOVE_E_WORKSPACE;
    if (int rc = plain_table(t, stream)) return rc;
    const bool behind = rest && packing_ok(p);
    const IdLaunch l = id_launch(c, c.sides, behind && (c.sides & 1) ? kFusePack : kFuseNone, behind && (c.sides & 2) ? kFusePack : kFuseNone);
#define CALL(LPR, NV)                                                                                                      \
    hipLaunchKernelGGL((pack_grad_kernel<LPR, NV>), dim3(l.nb), dim3(kBlock), 0, c.st, l.wk, l.rs, l.cs, c.d4, c.k, packed, \
                       c.w.blockpart, l.nb_row)
    GLOVE_DISPATCH_ROW_SHAPE(c.shape, CALL);
#undef CALL
    return (int)hipGetLastError();
}

int glove_pack_grad_f32(const glove_plan *p, const glove_tables *t, const glove_hyper *h, void *ws, size_t ws_bytes,
                        float *packed, int64_t capacity_entries, void *stream)
{
    return pack_ids(p, t, h, ws, ws_bytes, packed, capacity_entries, stream, false);
}

int glove_passes_packing_f32(const glove_plan *p, const glove_tables *t, const glove_hyper *h, void *ws, size_t ws_bytes,
                             float *packed, int64_t capacity_entries, void *stream)
{
    StepCall c;
    if (int rc = open_call(c, p, t, h, ws, ws_bytes, stream)) return rc;
    if (!packing_ok(p)) return passes_on_plain_table(c, PassOpts(c.sides));
    if (!packed) return GLOVE_E_BADARG;
    if (!packed_fits(c, capacity_entries)) return GLOVE_E_WORKSPACE;
    return passes_on_plain_table(c, PassOpts(c.sides).packing(packed));
}

int glove_pack_rest_f32(const glove_plan *p, const glove_tables *t, const glove_hyper *h, void *ws, size_t ws_bytes,
                        float *packed, int64_t capacity_entries, void *stream)
{
    return pack_ids(p, t, h, ws, ws_bytes, packed, capacity_entries, stream, true);
}

int glove_loss_partials_f32(const glove_plan *p, const glove_tables *t, void *ws, size_t ws_bytes, float *out4, void *stream)
{
    if (!p || !t || !ws || !out4 || t->d <= 0 || (t->d % 4) != 0) return GLOVE_E_BADARG;
    const StepWs w = carve_step_ws(ws, p->B, p->cap_chunks, t->d);
    if (w.bytes > ws_bytes) return GLOVE_E_WORKSPACE;
    const int lpr = pick_pass_shape(t->d / 4).lpr;
    if (lpr == 0) return GLOVE_E_BADARG;
    // the grid of the row pass that left them (folded by glove_rowside_step_adagrad_f32: any count reads the same)
    const int nb_row = packing_ok(p) ? fusepass_blocks(p, lpr, fuse_per(p, lpr), true) : rowpass_blocks(p, lpr);
    hipLaunchKernelGGL(loss_partials_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, w.blockpart, nb_row, out4);
    return (int)hipGetLastError();
}

static int packed_common(const glove_tables *t, float *G_flat, int32_t *mark, DenseViews &dv)
{
    if (!t || !G_flat || !mark || t->V <= 0 || t->d <= 0 || (t->d % 4) != 0) return GLOVE_E_BADARG;
    const int32_t Vr = v_row(t);
    const GradLayout L = grad_layout(Vr, t->V, t->d);
    dv = {G_flat + L.G_R, G_flat + L.G_br, G_flat + L.G_C, G_flat + L.G_bc, mark, (int)Vr};
    return pick_row_shape(t->d / 4).lpr == 0 ? GLOVE_E_BADARG : 0;
}

static bool to_list(const glove_packed_list *in, PackedList &out)
{
    if (!in || !in->entries || (!in->header && in->n < 0) || in->side < -1 || in->side > 1) return false;
    out = {in->entries, in->ids, in->header, (int)in->n, (int)in->side};
    return true;
}

// Every list is one a kernel can take: asked before the first launch over any of them
static int check_lists(const glove_packed_list *lists, int32_t n_lists)
{
    PackedList pl;
    for (int32_t i = 0; i < n_lists; ++i)
        if (!to_list(lists + i, pl)) return GLOVE_E_BADARG;
    return 0;
}

// The (checked) lists eight at a time, as a launch sees them: f(index of the batch's first list, the batch, the most entries one of
// its lists can hold — a list with a header holds up to capacity_entries)
extern "C++" template <class F>
static void for_each_list_batch(const glove_packed_list *lists, int32_t n_lists, int64_t capacity_entries, F f)
{
    for (int32_t first = 0; first < n_lists; first += 8) {
        PackedLists pls;
        pls.n = n_lists - first < 8 ? n_lists - first : 8;
        int64_t n_max = 0;
        for (int i = 0; i < pls.n; ++i) {
            to_list(lists + first + i, pls.l[i]);
            const int64_t n = pls.l[i].header ? capacity_entries : pls.l[i].n_host;
            n_max = n > n_max ? n : n_max;
        }
        f(first, pls, n_max);
    }
}

int glove_combine_packed_f32(const glove_packed_list *list, int32_t tag, const glove_tables *t, float *G_flat,
                             int32_t *mark, int64_t capacity_entries, void *stream)
{
    DenseViews dv;
    if (int rc = packed_common(t, G_flat, mark, dv)) return rc;
    PackedList pl;
    if (!to_list(list, pl) || tag < 0 || capacity_entries < 0) return GLOVE_E_BADARG;
    const int64_t n = pl.header ? capacity_entries : pl.n_host;
    if (n == 0) return 0;
    const int d4 = t->d / 4;
    const RowShape shape = pick_row_shape(d4);
    const int nb = blocks_for(n, kBlock / shape.lpr);
    hipStream_t st = (hipStream_t)stream;
#define CALL(LPR, NV) hipLaunchKernelGGL((combine_packed_kernel<LPR, NV>), dim3(nb), dim3(kBlock), 0, st, pl, (int)tag, dv, d4)
    GLOVE_DISPATCH_ROW_SHAPE(shape, CALL);
#undef CALL
    return (int)hipGetLastError();
}

int glove_count_packed_f32(const glove_packed_list *lists, int32_t n_lists, const glove_tables *t, float *G_flat,
                           int32_t *mark, int64_t capacity_entries, void *stream)
{
    DenseViews dv;
    if (int rc = packed_common(t, G_flat, mark, dv)) return rc;
    if (!lists || n_lists < 1 || n_lists > kMarkCountMask || capacity_entries < 0) return GLOVE_E_BADARG;
    if (int rc = check_lists(lists, n_lists)) return rc;
    const int d4 = t->d / 4;
    hipStream_t st = (hipStream_t)stream;
    for_each_list_batch(lists, n_lists, capacity_entries, [&](int32_t, const PackedLists &pls, int64_t n_max) {
        if (n_max > 0)
            hipLaunchKernelGGL(count_packed_kernel, dim3(blocks_for(n_max, kBlock), pls.n), dim3(kBlock), 0, st, pls, dv, d4);
    });
    return (int)hipGetLastError();
}

int glove_apply_packed_adagrad_f32(const glove_packed_list *lists, int32_t n_lists, const glove_tables *t,
                                   const glove_hyper *h, float *G_flat, int32_t *mark, const float *tail,
                                   float *loss_out, int64_t capacity_entries, void *stream)
{
    DenseViews dv;
    if (int rc = packed_common(t, G_flat, mark, dv)) return rc;
    if (!h || !lists || n_lists < 1 || capacity_entries < 0) return GLOVE_E_BADARG;
    if (!t->R || !t->C || !t->br || !t->bc || !t->scalars) return GLOVE_E_BADARG;
    // glove_hyper.optimizer: Adagrad, one of the per-row Keras optimizers (only touched rows move: the exchange is the same), or
    // a dense-decay one (Nadam, Adam, RMSprop: the sweep below moves the slots — Adam: the rows too — of every row no list names)
    const int opt = h->optimizer;
    const bool decays = opt == GLOVE_OPT_NADAM || opt == GLOVE_OPT_ADAM || opt == GLOVE_OPT_RMSPROP;
    if (int rc = check_optimizer(t, h, 3, opt)) return rc;
    if (h->sweep_sides < 0 || h->sweep_sides > 3) return GLOVE_E_BADARG;
    if (int rc = check_lists(lists, n_lists)) return rc;
    const OptHyper oh = opt_consts(h);
    const SlotTwo s2 = slot_two(t);
    if (int rc = plain_table(t, stream)) return rc;
    const int d4 = t->d / 4;
    const RowShape shape = pick_row_shape(d4);
    const StepConsts k = make_consts(t, h);
    SideBufs rs = {nullptr, nullptr, nullptr, t->R, t->s1_R, t->br, t->s1_br, nullptr, 0};
    SideBufs cs = {nullptr, nullptr, nullptr, t->C, t->s1_C, t->bc, t->s1_bc, nullptr, 0};
    hipStream_t st = (hipStream_t)stream;
    // the scalar work (global bias, loss) goes with the col side, like everywhere else; without an explicit tail it
    // sums the lists' headers in list order
    const int do_scalars = (sides_of(h) & 2) ? 1 : 0;
    float *scratch = nullptr;
    if (!tail && n_lists > 8 && do_scalars) {
        // a launch sees eight lists: sum the loss partials of all headers first (list order, so the sum is repeatable)
        scratch = G_flat + grad_layout(v_row(t), t->V, t->d).tail + 4;
        for_each_list_batch(lists, n_lists, capacity_entries, [&](int32_t first, const PackedLists &pls, int64_t) {
            hipLaunchKernelGGL(sum_headers_kernel, dim3(1), dim3(64), 0, st, pls, scratch, first == 0 ? 1 : 0);
        });
        tail = scratch;
    }
    if (decays) {
        // the rows nobody touched on the swept sides take their G = 0 update (the marks are still whole: the apply launches below
        // clear them as they go)
        const int sweep = h->sweep_sides ? h->sweep_sides : sides_of(h);
        const int lo = (sweep & 1) ? 0 : v_row(t), hi = (sweep & 2) ? v_row(t) + t->V : v_row(t);
        const int nbd = blocks_for(((int64_t)(hi - lo) + kSweepRows - 1) / kSweepRows, kBlock / shape.lpr);
#define CALL(LPR, NV)                                                                                                         \
        dispatch_opt<GLOVE_OPT_ADAM, GLOVE_OPT_RMSPROP, GLOVE_OPT_NADAM>(opt, [&](auto o_) {                                  \
            hipLaunchKernelGGL((decay_unmarked_kernel<LPR, NV, decltype(o_)::value>), dim3(nbd), dim3(kBlock), 0, st, dv, rs, cs, s2, \
                               d4, oh.b1, oh.b2, h->rho, h->learning_rate, h->epsilon, oh.ln_b1, oh.ln_b2,                    \
                               (const int64_t *)t->step, lo, hi);                                                             \
        })
        if (hi > lo) GLOVE_DISPATCH_ROW_SHAPE(shape, CALL);
#undef CALL
    }
    for_each_list_batch(lists, n_lists, capacity_entries, [&](int32_t first, const PackedLists &pls, int64_t n_max) {
        const int nbx = blocks_for(n_max > 0 ? n_max : 1, kBlock / shape.lpr);
        const int scal = first == 0 ? do_scalars : 0;
#define CALL(LPR, NV)                                                                                                         \
        dispatch_opt<GLOVE_OPT_ADAGRAD, GLOVE_OPT_SGD, GLOVE_OPT_ADAMAX, GLOVE_OPT_ADADELTA, GLOVE_OPT_NADAM, GLOVE_OPT_ADAM,  \
                     GLOVE_OPT_RMSPROP, GLOVE_OPT_FTRL, GLOVE_OPT_LAZYADAM, GLOVE_OPT_ROWWISE_ADAGRAD>(opt, [&](auto o_) {    \
            hipLaunchKernelGGL((apply_packed_kernel<LPR, NV, decltype(o_)::value>), dim3(nbx, pls.n), dim3(kBlock), 0, st, pls, dv, rs, \
                               cs, s2, d4, k, oh.o, oh.ln_b1, oh.ln_b2, (const int64_t *)t->step, (int)first, tail, t->scalars,    \
                               loss_out, scal);                                                                               \
        })
        GLOVE_DISPATCH_ROW_SHAPE(shape, CALL);      // (packed_common has seen the shape: the macro's own refusal cannot come)
#undef CALL
        return 0;
    });
    if (scratch) {
        hipError_t e = zero_words(scratch, 4, st);      // the tail is all zero between steps
        if (e != hipSuccess) return (int)e;
    }
    return (int)hipGetLastError();
}

int glove_gather_rows_f32(const float *W, const float *bias, const int32_t *ids, int32_t n, int32_t d, float *rows,
                          float *biases, void *stream)
{
    if (n < 0 || d <= 0 || (d % 4) != 0) return GLOVE_E_BADARG;
    if (n == 0) return 0;
    if (!W || !bias || !ids || !rows || !biases) return GLOVE_E_BADARG;
    const int d4 = d / 4;
    const RowShape shape = pick_row_shape(d4);
    if (shape.lpr == 0) return GLOVE_E_BADARG;
    const int nb = blocks_for(n, kBlock / shape.lpr);
    hipStream_t st = (hipStream_t)stream;
#define CALL(LPR, NV) hipLaunchKernelGGL((gather_rows_kernel<LPR, NV>), dim3(nb), dim3(kBlock), 0, st, W, bias, ids, (int)n, d4, rows, biases)
    GLOVE_DISPATCH_ROW_SHAPE(shape, CALL);
#undef CALL
    return (int)hipGetLastError();
}

// Forms 1 / 3 / 4 on the same resident plans, one process, interleaved rounds (tools/ab_step_forms.py, round 4; us per step):
//   V = 50 k,  d = 300 (table 61 MB):  146 MB of touched rows  71.0 /  70.7 /  72.8    221 MB 105.9 / 101.0 / 103.2    311 MB 175.3 / 152.5 / 153.0
//   V = 400 k, d = 300 (486 MB):       226 MB 102.5 / 104.8 /  98.7                    388 MB 178.2 / 163.6 / 151.9    649 MB 333.0 / 277.1 / 247.5
//   V = 2 M,   d = 128 (1 GB):         209 MB 128.6 / 122.9 / 120.6                    368 MB 220.3 / 199.4 / 188.8
//   V = 10 k,  d = 64, B = 1 M (20 MB touched): 55.2 / 82.3 / 87.7
// A tie at 146 MB, 4 - 6 % for the fused forms from 209 MB on (the twin form on tables beyond the Infinity Cache, the
// three-launch form on the 61 MB table): the switch sat between (192 MB).
// Round 5 (the passes compiled for one head, staged version lookups, six chunks per lane group; same tool, forms 1 / 3 / 4):
//   V = 50 k,  d = 300:  56 MB 32.5 / 39.1 / 40.8     75 MB 41.1 / 41.6 / 42.8     92 MB 46.2 / 44.3 / 46.5    122 MB 57.6 / 54.4 / 58.5   148 MB 69.2 / 62.5 / 67.5
//   V = 400 k, d = 300:  77 MB 42.2 / 44.2 / 46.5    137 MB 60.3 / 58.0 / 60.9    241 MB 98.3 / 93.5 / 89.6
//   V = 2 M,   d = 128:  35 MB 26.0 / 31.8 / 35.9     64 MB 42.2 / 40.2 / 41.8    117 MB 67.5 / 63.9 / 63.1    209 MB 114.3 / 114.4 / 104.5
// The fused forms now pay from 90 MB on: the switch is GLOVE_FUSED_STEP_BYTES = 96 MB.

// Which form a sparse Adagrad step takes (glove_hyper.step_form; see include/glove_hip.h).
static int pick_step_form(const glove_plan *p, const glove_tables *t, const glove_hyper *h)
{
    if (!p || !t || !h) return GLOVE_STEP_TWO_LAUNCH;
    if (sides_of(h) != 3) return GLOVE_STEP_TWO_LAUNCH;
    // the fused forms read the id layout from the chunk records, or from the run words of a plan that keeps pair arrays instead
    const bool records = p->r_crec && p->c_crec;
    const bool run_words = p->r_chunk_hw && p->c_chunk_hw && p->r_partner && p->r_w && p->r_y && p->c_partner && p->c_w && p->c_y;
    if (!records && !run_words) return GLOVE_STEP_TWO_LAUNCH;
    if (!records && h->step_form == GLOVE_STEP_TAGGED) return GLOVE_STEP_TWO_LAUNCH;        // (the one-launch form walks records)
    if (h->step_form != GLOVE_STEP_AUTO) return h->step_form;
    // the latency-bound regime on step-tagged tables: everything in one launch
    // ... unless the batch is known to hold heavy ids (more than plan.heavy_chunks chunks: a frequent token with hundreds of the
    // batch's pairs): the tagged form walks ALL chunks of an id in one lane group, one record trip after the other, and beyond
    // heavy_chunks its summation order is no longer the two-launch form's.  (A plan refilled on the device keeps its counts
    // there: host_counts[4] < 0, judged by the batch size alone.)
    if (t->R_tag && t->C_tag && p->B <= 2048 && records && p->host_counts[4] <= 0) return GLOVE_STEP_TAGGED;     // (measured against the two-launch form, 64 staging plans: 512 / 1,024 / 2,048 pairs -16 / -16 / -13 %, 4,096 +12 %)
    // the fused forms pay off once the touched rows and their partials no longer live in the caches; the id counts
    // are known on the host for a plan whose build has been synchronised (a resident plan)
    // (a plan refilled on the device every step — a reshuffled epoch — is judged by the most ids its batch can hold)
    const int64_t most = (int64_t)v_row(t) + t->V < 2 * p->B ? (int64_t)v_row(t) + t->V : 2 * p->B;
    const int64_t ids = p->host_counts[1] >= 0 && p->host_counts[3] >= 0 ? (int64_t)p->host_counts[1] + p->host_counts[3] : most;
    // (V = 50 k, d = 300, B = 131,072: 48 k ids = 230 MB per step, all of it living in the Infinity Cache: two launches
    // 106 us, fused 103 - 111; V = 400 k at B = 131,072, 336 MB: 172 against 156; V = 50 k at B = 1 M, 432 MB: 378 against 314)
    if (ids * t->d * 16 < (int64_t)GLOVE_FUSED_STEP_BYTES) return GLOVE_STEP_TWO_LAUNCH;        // (the table of measurements above)
    return t->R_ver ? GLOVE_STEP_FUSED_TWIN : GLOVE_STEP_FUSED_THREE_LAUNCH;
}

// Whether an Adam step takes the one-launch form (tagged_adam_kernel): twinned tables (glove_tables.R_tag / C_tag are the
// sign; the tags themselves stay zero), a plan with chunk records and id bitmaps, a small batch that touches a minority of the rows
static bool adam_one_launch(const glove_plan *p, const glove_tables *t, const glove_hyper *h)
{
    if (!p || !t || !h || sides_of(h) != 3) return false;
    if (!t->R_tag || !t->C_tag || !p->r_crec || !p->c_crec || !p->r_mark || !p->c_mark) return false;
    if (h->step_form != GLOVE_STEP_AUTO && h->step_form != GLOVE_STEP_TAGGED) return false;
    if (h->step_form == GLOVE_STEP_AUTO && p->host_counts[4] > 0) return false;     // heavy ids: as pick_step_form
    return p->B <= 2048 && 2 * p->B <= (int64_t)v_row(t) + t->V;
}

// n consecutive one-launch steps (opt: GLOVE_OPT_ADAGRAD on step-tagged tables, GLOVE_OPT_ADAM on twins flipped as a whole) as
// chains: one launch per step, the global bias handed from step to step through chain records in the workspace (the one-launch
// forms keep nothing else there: no partial rows), one epilogue launch per chain.
static int launch_tagged_chain(const glove_plan *const *plans, int n, const glove_tables *t, const glove_hyper *h, void *ws,
                               size_t ws_bytes, float *loss_out, void *stream, int opt)
{
    if (!plans || n < 1 || !t || !h || !ws) return GLOVE_E_BADARG;
    const bool adam = opt == GLOVE_OPT_ADAM;
    StepCall c;         // one per plan; behind the loop the last one's, of which the launches take what no plan changes
    int most_blocks = 1;
    for (int i = 0; i < n; ++i) {
        const glove_plan *p = plans[i];
        if (int rc = open_call(c, p, t, h, ws, ws_bytes, stream, false)) return rc;       // (the workspace holds chain records)
        if (adam ? !adam_one_launch(p, t, h) : (!t->R_tag || !t->C_tag || !p->r_crec || !p->c_crec)) return GLOVE_E_BADARG;
        const int rb = rowpass_blocks(p, c.pass.lpr);
        most_blocks = rb > most_blocks ? rb : most_blocks;
    }
    if (c.sides != 3) return GLOVE_E_BADARG;
    if (int rc = check_optimizer(t, h, 3, opt)) return rc;
    const size_t rec_floats = (size_t)kChainHead + (size_t)kPartials * most_blocks;
    const size_t fit = ws_bytes / (rec_floats * sizeof(float));
    if (fit < 1) return GLOVE_E_WORKSPACE;
    const int d4 = c.d4;
    const RowShape shape = c.pass;
    const StepConsts &kc = c.k;
    const OptHyper oh = opt_consts(h);
    hipStream_t st = c.st;
    float *recs = (float *)ws;
    // Adam's sweep over all other rows: its part of the grid as adam_fused_kernel's, behind a multiple of 8 workgroups, so that
    // every step's sweep finds the rows it wrote last step in the same L2s
    const int sweep_rows = tagged_sweep_rows(shape.nv);
    const int sweep_blocks = adam ? blocks_for(((int64_t)v_row(t) + t->V + sweep_rows - 1) / sweep_rows, kBlock / shape.lpr) : 0;
    for (int i0 = 0; i0 < n; i0 += (int)fit) {
        const int m = n - i0 < (int)fit ? n - i0 : (int)fit;
        int prev_blocks = 0;
        for (int i = 0; i < m; ++i) {
            const glove_plan *p = plans[i0 + i];
            // the classic passes' grid and chunk assignment
            const int row_blocks = rowpass_blocks(p, shape.lpr), chunk_blocks = adam ? (2 * row_blocks + 7) & ~7 : 2 * row_blocks;
            const int nb = chunk_blocks + sweep_blocks;
            const float *prev = i > 0 ? recs + (size_t)(i - 1) * rec_floats : nullptr;
            float *mine = recs + (size_t)i * rec_floats;
#define CALL(LPR, NV)                                                                                                           \
            dispatch_bool(LPR * NV == d4, [&](auto full) {                                                                      \
                constexpr bool FULL = decltype(full)::value;                                                                    \
                if (adam)                                                                                                       \
                    hipLaunchKernelGGL((tagged_adam_kernel<LPR, NV, FULL>), dim3(nb), dim3(kBlock), 0, st, p->counts,           \
                                       step_side<AdamSide>(p, t, true), step_side<AdamSide>(p, t, false), row_blocks,           \
                                       chunk_blocks, (const float *)t->scalars, (const int64_t *)t->step, d4, h->inv_batch, (int)h->head, \
                                       h->neg_factor, kc, oh.b1, oh.b2, oh.ln_b1, oh.ln_b2, prev, prev_blocks, mine, i);        \
                else                                                                                                            \
                    hipLaunchKernelGGL((tagged_step_kernel<LPR, NV, FULL>), dim3(nb), dim3(kBlock), 0, st, p->counts,           \
                                       step_side<OneSide>(p, t, true), step_side<OneSide>(p, t, false), row_blocks,             \
                                       (const float *)t->scalars, (const int64_t *)t->step, d4, h->inv_batch, (int)h->head,    \
                                       h->neg_factor, kc, prev, prev_blocks, mine, i);                                         \
            })
            GLOVE_DISPATCH_PASS_SHAPE(shape, CALL);
#undef CALL
            prev_blocks = row_blocks;
        }
        const float *last = recs + (size_t)(m - 1) * rec_floats;
        dispatch_opt<GLOVE_OPT_ADAGRAD, GLOVE_OPT_ADAM>(opt, [&](auto o_) {
            hipLaunchKernelGGL((tagged_flush_kernel<decltype(o_)::value>), dim3(1), dim3(kBlock), 0, st, t->scalars, t->step, last, prev_blocks,
                               m, kc, oh.b1, oh.b2, oh.ln_b1, oh.ln_b2, i0 + m == n ? loss_out : nullptr);
        });
    }
    return (int)hipGetLastError();
}

int glove_step_adagrad_f32(const glove_plan *p, const glove_tables *t, const glove_hyper *h, void *ws, size_t ws_bytes,
                           float *loss_out, void *stream)
{
    const int form = pick_step_form(p, t, h);
    if (form == GLOVE_STEP_TAGGED) return launch_tagged_chain(&p, 1, t, h, ws, ws_bytes, loss_out, stream, GLOVE_OPT_ADAGRAD);
    StepCall c;
    if (int rc = open_call(c, p, t, h, ws, ws_bytes, stream)) return rc;
    // every form ends in the apply launch, which needs the slots; the twin form needs the version bytes
    if (form < GLOVE_STEP_TWO_LAUNCH || form > GLOVE_STEP_FUSED_TWIN || !has_slot1(t)) return GLOVE_E_BADARG;
    if (form == GLOVE_STEP_FUSED_TWIN && !t->R_ver) return GLOVE_E_BADARG;
    // only the twin form follows the version bytes of a twinned row table: every other form first brings it home
    // (a step of another form behind a twin step would otherwise read and write copy 0 of rows whose current copy is the second)
    if (form != GLOVE_STEP_FUSED_TWIN)
        if (int rc = plain_table(t, stream)) return rc;
    switch (form) {
    case GLOVE_STEP_FUSED_ONE_PASS:
        // (tests / comparisons) both sides in one launch: neither table may change under the other side's gathers, so both put
        // their finished rows into the slots and the apply launch moves them
        if (int rc = launch_passes(c, PassOpts(3).fuse(kFuseSlot, kFuseSlot))) return rc;
        return launch_apply_adagrad(c, loss_out, kFuseSlot, kFuseSlot);
    case GLOVE_STEP_FUSED_THREE_LAUNCH:
        // row side first (C is read only); then the col side alone may update C in place while it gathers the
        // still unchanged R; the apply launch moves the row side's finished rows and does the multi-chunk ids
        if (int rc = launch_passes(c, PassOpts(1).fuse(kFuseSlot, kFuseNone))) return rc;
        if (int rc = launch_passes(c, PassOpts(2).fuse(kFuseNone, kFuseInPlace))) return rc;
        return launch_apply_adagrad(c, loss_out, kFuseSlot, kFuseInPlace);
    case GLOVE_STEP_FUSED_TWIN: {
        // as the three-launch form, but the row side writes its new rows into the other copy of the twinned row table:
        // the col side keeps gathering the old rows from the current copy, and the apply launch only flips versions
        if (int rc = launch_passes(c, PassOpts(1).fuse(kFuseTwin, kFuseNone).on_twin())) return rc;
        // (the list of ids for the apply launch rides in the col-side launch when both sides step and the workspace has the list)
        const bool tail = c.w.work != nullptr && c.sides == 3;
        if (int rc = launch_passes(c, PassOpts(2).fuse(kFuseNone, kFuseInPlace).on_twin(tail))) return rc;
        return launch_apply_adagrad(c, loss_out, kFuseTwin, kFuseInPlace, tail);
    }
    default:        // GLOVE_STEP_TWO_LAUNCH
        if (int rc = launch_passes(c, PassOpts(3))) return rc;
        return launch_apply_adagrad(c, loss_out, kFuseNone, kFuseNone);
    }
}

int glove_rowside_step_adagrad_f32(const glove_plan *p, const glove_tables *t, const glove_hyper *h, void *ws, size_t ws_bytes,
                                   void *stream)
{
    StepCall c;
    if (int rc = open_call(c, p, t, h, ws, ws_bytes, stream)) return rc;
    if (c.sides != 1 || !has_slot1(t)) return GLOVE_E_BADARG;              // hyper.sides = 1: this is the row side's step
    if (int rc = plain_table(t, stream)) return rc;
    if (!p->r_crec || !p->c_crec) {
        // no chunk records: the row pass stores its partial rows, the apply launch does every row id
        if (int rc = launch_passes(c, PassOpts(1))) return rc;
        return launch_apply_adagrad(c, nullptr, kFuseNone, kFuseNone);
    }
    if (int rc = launch_passes(c, PassOpts(1).fuse(kFuseInPlace, kFuseNone))) return rc;
    if (int rc = launch_apply_adagrad(c, nullptr, kFuseInPlace, kFuseNone)) return rc;
    const int nb_fused = fusepass_blocks(p, c.pass.lpr, fuse_per(p, c.pass.lpr), true);
    hipLaunchKernelGGL(fold_blockpart_kernel, dim3(1), dim3(kBlock), 0, c.st, c.w.blockpart, nb_fused);
    return (int)hipGetLastError();
}

int glove_canonicalize_f32(const glove_tables *t, void *stream)
{
    if (!t || !t->R || !t->br || t->V <= 0 || t->d <= 0 || (t->d % 4) != 0) return GLOVE_E_BADARG;
    if (!t->R_ver && !t->R_tag) return 0;
    const int d4 = t->d / 4;
    const RowShape shape = pick_row_shape(d4);
    if (shape.lpr == 0) return GLOVE_E_BADARG;
    const int Vr = v_row(t);
    const int nb = blocks_for(Vr, kBlock / shape.lpr);
    hipStream_t st = (hipStream_t)stream;
    if (t->R_tag) {                             // step-tagged twins of both tables (the one-launch step)
        if (!t->C_tag || !t->C || !t->bc || t->R_ver) return GLOVE_E_BADARG;
        const int nbc = blocks_for(t->V, kBlock / shape.lpr);
#define CALL(LPR, NV)                                                                                                  \
        hipLaunchKernelGGL((untag_kernel<LPR, NV>), dim3(nb), dim3(kBlock), 0, st, t->R, t->br, t->R_tag, Vr, d4);     \
        hipLaunchKernelGGL((untag_kernel<LPR, NV>), dim3(nbc), dim3(kBlock), 0, st, t->C, t->bc, t->C_tag, (int)t->V, d4)
        GLOVE_DISPATCH_ROW_SHAPE(shape, CALL);
#undef CALL
        // the one-launch Adam step flips the tables as a whole (scalars[3]) instead of tagging rows
        if (t->scalars) {
#define CALL(LPR, NV)                                                                                                  \
            hipLaunchKernelGGL((twin_home_kernel<LPR, NV>), dim3(nb), dim3(kBlock), 0, st, t->R, t->br, (const float *)t->scalars, Vr, d4);  \
            hipLaunchKernelGGL((twin_home_kernel<LPR, NV>), dim3(nbc), dim3(kBlock), 0, st, t->C, t->bc, (const float *)t->scalars, (int)t->V, d4)
            GLOVE_DISPATCH_ROW_SHAPE(shape, CALL);
#undef CALL
            hipLaunchKernelGGL(twin_home_done_kernel, dim3(1), dim3(64), 0, st, t->scalars);
        }
        return (int)hipGetLastError();
    }
#define CALL(LPR, NV) hipLaunchKernelGGL((canonicalize_kernel<LPR, NV>), dim3(nb), dim3(kBlock), 0, st, t->R, t->br, t->R_ver, Vr, d4)
    GLOVE_DISPATCH_ROW_SHAPE(shape, CALL);
#undef CALL
    return (int)hipGetLastError();
}

// n steps on one set of tables: runs of consecutive steps that take the one-launch form of `opt` (`chained` says so of a plan) go
// out as chains, one launch per step (launch_tagged_chain); every other step on its own (`single`); the last one writes loss_out
extern "C++" template <class Chained, class Single>
static int steps_in_chains(const glove_plan *const *plans, int32_t n, const glove_tables *t, const glove_hyper *h, void *ws,
                           size_t ws_bytes, float *loss_out, void *stream, int opt, Chained chained, Single single)
{
    if (!plans || n < 0) return GLOVE_E_BADARG;
    for (int32_t i = 0; i < n;) {
        int32_t k = i;
        while (k < n && chained(plans[k])) ++k;
        if (k > i) {
            if (int rc = launch_tagged_chain(plans + i, k - i, t, h, ws, ws_bytes, k == n ? loss_out : nullptr, stream, opt)) return rc;
            i = k;
            continue;
        }
        if (int rc = single(plans[i], i == n - 1 ? loss_out : nullptr)) return rc;
        ++i;
    }
    return 0;
}

int glove_steps_adagrad_f32(const glove_plan *const *plans, int32_t n, const glove_tables *t, const glove_hyper *h,
                            void *ws, size_t ws_bytes, float *loss_out, void *stream)
{
    return steps_in_chains(plans, n, t, h, ws, ws_bytes, loss_out, stream, GLOVE_OPT_ADAGRAD,
                           [&](const glove_plan *p) { return pick_step_form(p, t, h) == GLOVE_STEP_TAGGED; },
                           [&](const glove_plan *p, float *loss) { return glove_step_adagrad_f32(p, t, h, ws, ws_bytes, loss, stream); });
}

// passes (marking the batch's ids) + adam_fused_kernel: see the kernel's header.  which = 1: the row side alone (the row pass,
// the row ids' apply, the sweep over R's rows; no scalar work — glove_rowside_step_f32, whose G_flat IS the V_row marks), 3: both
// sides (the marks in G_flat's bias segments)
static int step_adam_fused(const StepCall &c, float *G_flat, float *loss_out, bool nadam = false, int which = 3)
{
    const glove_tables *t = c.t;
    if (!G_flat) return GLOVE_E_BADARG;
    if (int rc = check_optimizer(t, c.h, 3, nadam ? GLOVE_OPT_NADAM : GLOVE_OPT_ADAM)) return rc;     // (both sides' slots, whichever step)
    if (int rc = plain_table(t, c.st)) return rc;
    const int32_t Vr = v_row(t);
    const GradLayout L = grad_layout(Vr, t->V, t->d);
    float *mark_rows = which & 2 ? G_flat + L.G_br : G_flat, *mark_cols = which & 2 ? G_flat + L.G_bc : nullptr;
    if (int rc = launch_passes(c, PassOpts(which).marks(mark_rows, mark_cols))) return rc;
    const IdLaunch l = id_launch(c, which);
    const int32_t Vc = which & 2 ? t->V : 0;         // col rows the sweep covers (behind R's rows)
    // a multiple of 8 workgroups in front: workgroups b and b + 8 share an XCD, so every step's sweep then finds
    // the rows it wrote last step in the same L2s, whatever the batch's id count (5.3 vs 11 us per launch)
    const int nb_apply = (l.nb + 7) & ~7;
    const int nb = nb_apply + blocks_for(((int64_t)Vr + Vc + kSweepRows - 1) / kSweepRows, kBlock / c.shape.lpr);
    const OptHyper oh = opt_consts(c.h);
#define CALL(LPR, NV)                                                                                                  \
    dispatch_opt<GLOVE_OPT_ADAM, GLOVE_OPT_NADAM>(nadam ? GLOVE_OPT_NADAM : GLOVE_OPT_ADAM, [&](auto o_) {            \
        hipLaunchKernelGGL((adam_fused_kernel<LPR, NV, decltype(o_)::value>), dim3(nb), dim3(kBlock), 0, c.st, l.wk, l.rs, l.cs, slot_two(t), \
                           c.d4, c.k, oh.b1, oh.b2, oh.ln_b1, oh.ln_b2, (const int64_t *)t->step, t->scalars,         \
                           (const float *)c.w.blockpart, l.nb_row, mark_rows, mark_cols, (int)Vr, (int)Vc, nb_apply, loss_out); \
    })
    GLOVE_DISPATCH_ROW_SHAPE(c.shape, CALL);
#undef CALL
    if (which == 1)         // the row pass's loss partials, folded: any later reader finds them whatever grid it assumes
        hipLaunchKernelGGL(fold_blockpart_kernel, dim3(1), dim3(kBlock), 0, c.st, c.w.blockpart, l.nb_row);
    return (int)hipGetLastError();
}

int glove_step_adam_f32(const glove_plan *p, const glove_tables *t, const glove_hyper *h, void *ws, size_t ws_bytes,
                        float *G_flat, float *loss_out, void *stream)
{
    if (adam_one_launch(p, t, h)) return launch_tagged_chain(&p, 1, t, h, ws, ws_bytes, loss_out, stream, GLOVE_OPT_ADAM);
    // a batch that touches a minority of the rows (the reference's 1,024 pairs): two launches, no gradient buffer
    // traffic; a batch that touches most rows: the dense form, whose sweep then wastes nothing
    StepCall c;
    if (int rc = open_call(c, p, t, h, ws, ws_bytes, stream)) return rc;
    if (c.sides == 3 && 2 * p->B <= (int64_t)v_row(t) + t->V) return step_adam_fused(c, G_flat, loss_out);
    return dense_step(c, 3, G_flat, loss_out);
}

// A step of the per-row optimizers (SGD, Adamax, Adadelta, Ftrl, LazyAdam, RowWiseAdagrad): the passes of `sides`, then apply_sparse_opt_kernel on their ids
// (1: the row ids alone, no scalar work)
static int launch_sparse_opt_step(const StepCall &c, int sides, float *loss_out)
{
    const glove_tables *t = c.t;
    const int opt = c.h->optimizer;
    if (opt != GLOVE_OPT_SGD && opt != GLOVE_OPT_ADAMAX && opt != GLOVE_OPT_ADADELTA && opt != GLOVE_OPT_FTRL && opt != GLOVE_OPT_LAZYADAM &&
        opt != GLOVE_OPT_ROWWISE_ADAGRAD)
        return GLOVE_E_BADARG;
    if (int rc = plain_table(t, c.st)) return rc;
    if (int rc = launch_passes(c, PassOpts(sides))) return rc;
    const IdLaunch l = id_launch(c, sides);
    const OptHyper oh = opt_consts(c.h);
#define CALL(LPR, NV)                                                                                                      \
    dispatch_opt<GLOVE_OPT_SGD, GLOVE_OPT_ADAMAX, GLOVE_OPT_ADADELTA, GLOVE_OPT_FTRL, GLOVE_OPT_LAZYADAM,                  \
                 GLOVE_OPT_ROWWISE_ADAGRAD>(opt, [&](auto o_) {                                                           \
        hipLaunchKernelGGL((apply_sparse_opt_kernel<LPR, NV, decltype(o_)::value>), dim3(l.nb), dim3(kBlock), 0, c.st, l.wk, l.rs, l.cs, \
                           slot_two(t), c.d4, c.k, oh.o, oh.ln_b1, oh.ln_b2, (const int64_t *)t->step, t->scalars,        \
                           (const float *)c.w.blockpart, l.nb_row, loss_out);                                             \
    })
    GLOVE_DISPATCH_ROW_SHAPE(c.shape, CALL);
#undef CALL
    return (int)hipGetLastError();
}

int glove_step_sparse_f32(const glove_plan *p, const glove_tables *t, const glove_hyper *h, void *ws, size_t ws_bytes,
                          float *G_flat, float *loss_out, void *stream)
{
    if (!h) return GLOVE_E_BADARG;
    if (h->optimizer == GLOVE_OPT_ADAGRAD) return glove_step_adagrad_f32(p, t, h, ws, ws_bytes, loss_out, stream);
    if (h->optimizer == GLOVE_OPT_ADAM) return glove_step_adam_f32(p, t, h, ws, ws_bytes, G_flat, loss_out, stream);
    StepCall c;
    if (int rc = open_call(c, p, t, h, ws, ws_bytes, stream)) return rc;
    if (c.sides != 3) return GLOVE_E_BADARG;
    if (int rc = check_optimizer(t, h, 3, h->optimizer)) return rc;
    if (h->optimizer == GLOVE_OPT_NADAM)        // passes (marking the batch's ids) + one kernel: apply for the ids, decay of m and v for all other rows
        return step_adam_fused(c, G_flat, loss_out, true);
    if (h->optimizer == GLOVE_OPT_RMSPROP) return dense_step(c, 3, G_flat, loss_out);
    return launch_sparse_opt_step(c, 3, loss_out);
}

int glove_rowside_step_f32(const glove_plan *p, const glove_tables *t, const glove_hyper *h, void *ws, size_t ws_bytes,
                           float *G_flat, void *stream)
{
    if (!h) return GLOVE_E_BADARG;
    if (h->optimizer == GLOVE_OPT_ADAGRAD) return glove_rowside_step_adagrad_f32(p, t, h, ws, ws_bytes, stream);
    StepCall c;
    if (int rc = open_call(c, p, t, h, ws, ws_bytes, stream)) return rc;
    if (c.sides != 1) return GLOVE_E_BADARG;                                 // hyper.sides = 1: this is the row side's step
    if (!t->s1_R || !t->s1_br) return GLOVE_E_BADARG;
    const int opt = h->optimizer;
    if (opt == GLOVE_OPT_ADAM || opt == GLOVE_OPT_NADAM)
        // the row pass marks the batch's row ids; one kernel applies them and gives every other row of the shard its G = 0 update
        return step_adam_fused(c, G_flat, nullptr, opt == GLOVE_OPT_NADAM, 1);
    if (int rc = check_optimizer(t, h, 1, opt)) return rc;
    if (opt == GLOVE_OPT_RMSPROP) {
        // the row half of glove_step_sparse_f32's RMSprop: the summed row gradients into G_flat, the sweep over R's rms slot
        if (int rc = dense_step(c, 1, G_flat, nullptr)) return rc;
    } else {
        // the per-row optimizers: the row pass, then their epilogue on the row ids (apply_sparse_opt_kernel, sides 1: no scalar work)
        if (int rc = launch_sparse_opt_step(c, 1, nullptr)) return rc;
    }
    // the row pass's loss partials, folded: glove_loss_partials_f32 / the col side's dense gradient find them whatever grid they assume
    hipLaunchKernelGGL(fold_blockpart_kernel, dim3(1), dim3(kBlock), 0, c.st, c.w.blockpart, rowpass_blocks(p, c.pass.lpr));
    return (int)hipGetLastError();
}

int glove_steps_adam_f32(const glove_plan *const *plans, int32_t n, const glove_tables *t, const glove_hyper *h,
                         void *ws, size_t ws_bytes, float *G_flat, float *loss_out, void *stream)
{
    return steps_in_chains(plans, n, t, h, ws, ws_bytes, loss_out, stream, GLOVE_OPT_ADAM,
                           [&](const glove_plan *p) { return adam_one_launch(p, t, h); },
                           [&](const glove_plan *p, float *loss) { return glove_step_adam_f32(p, t, h, ws, ws_bytes, G_flat, loss, stream); });
}


}  // extern "C"

// scan_screen.hip -- fp16 SCREENING scan + exact fp32 re-scoring (gfx950 / MI355X only).
//
// Same job as scan_topk.hip (the FLAT search behind server/RAGHelper.py:497-499) at a fraction of the MFMA time, and
// still exact: the screen only PROPOSES candidates; the returned ids/scores come from an fp32 re-score in the
// exact kernel's own summation order, guarded by a per-query sufficiency test; queries that fail it are answered
// by the exact scan.
//
// Screening image (built at add time, HALF the bytes of the fp32 matrix: 768 B per 384-d row): h = fp16(64 * x) in
// natural k order (the 2^6 scale keeps |x| >= 1e-6 out of the fp16 subnormal range; |x| must stay below ~1000).
// Queries are converted the same way per call.
//   4096 * s~ = sum h_x . h_q                    (one fp32 accumulator per score: 24 accumulations of 16 k by v_mfma_f32_32x32x16_f16 in the
//                                                 4-wave kernels, 12 of 32 k by v_mfma_f32_16x16x32_f16 in the 8-wave ones)
// Error vs the exact kernel's fp32 score, with dx = x - h_x/64 (row), dq = q - h_q/64 (query), by Cauchy-Schwarz:
//   |sum (x q - h_x h_q)/4096| <= |dx| |q| + |x| |dq| + |dx| |dq|.
// |dx|max is MEASURED when rows are added (k_img_err; ~1.7e-4 |x| for real data, 4.9e-4 |x| worst case) and |dq| is
// measured per query in the re-score kernel, so subnormal flushes and odd value ranges are covered by construction.
// The fp32 accumulation of 384 exact fp16 products adds <= 408 * 2^-24 = 2.5e-5 |x||q| (the 8-wave kernels round 12 partial sums of 32 k into
// the accumulator where the 4-wave ones round 24 of 16 k: inside the same budget) and the exact kernel is itself
// within 384 * 2^-24 = 2.3e-5 |x||q| of the true dot product:
//   EPS(q) = |dx|max |q| + |x|max |dq| + |dx|max |dq| + 5e-5 |x|max |q|          (~4e-4 for unit vectors)
// Sufficiency (per query): with the approximate top-K' (K' = 32) sorted, tau = k-th best s~.  If fewer than K'
// candidates exist, or s~[K'-1] < tau - 2*EPS, every row outside the candidate set has an exact score below k rows
// of the set, so the exact top-k is inside it.  Otherwise the query is flagged and re-run on the exact scan.
// Band seeding (the threshold ladder of rmu_api.hip: screen_enqueue): K' exists only so that the test above can pass, and a row that is
// below the test's lower edge when it is seen can neither be in the exact top-k nor change the test's outcome.  So the merge that seeds a
// launch (topk_merge.hip: seed_band) publishes, beside the K'-th key, the image of tau_now - 2 EPS (1 + 2^-10) rounded one key step down
// (tau_now = the k-th best approximate score so far; EPS(q) is computed by the query conversion with the re-score kernel's own arithmetic:
// screen_eps); the launch's threshold is the larger of the two.  Given: the filter is strict (p > thr), thresholds only rise, tau only rises,
// so a dropped row had s~ <= thr_level <= max(final K'-th, tau_final - 2 EPS (1 + guard)).
//   Dropped below the K'-th: the argument above, unchanged.
//   Dropped below the band: its exact score is <= s~ + EPS < tau_final - EPS (strictly: the guard and the key step), and each of the k best
//   approximate candidates has an exact score >= tau_final - EPS: k rows beat it outright, the row-id tie rule never gets to decide.
//   Flagging: a query is flagged iff at least K' rows have s~ >= tau_final - 2 EPS.  fl(tau_now - 2 EPS (1 + 2^-10)) <= fl(tau_final - 2 EPS)
//   (rounding is monotone; the guard also covers an EPS that differs from the re-score kernel's in its last bits), one key step below it is
//   strictly less, so every such row passes every level's threshold and is kept: the same queries are flagged with the band and without.
// The band is published only when the merged K'-th key exists ("fewer than K' candidates" must go on meaning that every live row is one),
// when EPS is finite, and when k < K' (rmu_index_screen_candidates asks for k = K' and still gets the true approximate top-K').
// RMU_OPT_SCREEN_BAND = 0 seeds the K'-th key alone.  On random unit rows the band's edge sits near rank 11-12 of K' = 32 at k = 10: a seeded
// level appends about a third of the K' (ratio - 1) candidates per query it appended before (tests/test_screen_band_cpu.py: 0.34).
// Spill path (RMU_OPT_SCREEN_SPILL; the SEEDED launches of the 8-wave kernels): a tile in which some lane passes used to enter slow_path --
// owner change, a walk over the rows, an exchange with the partner lane per row, per-query slot counts, scattered 8-byte stores -- while the
// workgroup's other seven waves wait for that wave at the pair barrier.  None of that per-query work has to happen there.  A lane whose
// running maximum beats its group's threshold stores the 8 scores it holds of that group, in the MFMA's own layout, with (tile, lane, group)
// into a list of its wave (spill_tile below), and a sift kernel behind the launch (topk_merge.hip: sift_kernel) decides which query and row a
// score belongs to and whether it survives.  Why deferring is sound: in a seeded launch a query's threshold is the word the last merge
// published (gthr[q]); only a compaction raises it during the launch, to some chunk's own K'-th best, and thresholds only rise.  The lane
// spilled because its maximum beat the threshold of that moment; the sift tests every score of the record, strictly, against gthr[q] as it
// stands after the launch -- the same word or a higher one.  So the sift keeps exactly {rows of the range with s~ > gthr[q]}; an append
// would have kept a superset of the best K' of that set and the merge would have cut it to those.  A score the sift drops for a raised
// threshold is below K' rows of this range, as with appends: nothing is dropped that an append would have kept in the merged top-K'.  The
// merged keys, their order and the seeds of the next launch (K'-th key and band edge: seed_band, unchanged) are the same, bit for bit.
// A list holds spill_cap records; a wave whose list cannot take a tile's records takes slow_path for that tile and every later one, its
// slots are emitted as before and the sift folds that part list in (RMU_SPILL_FELL in the wave's count word).  The cold first launch, its
// direct path, its raw emit and the unsorted merge are untouched, and so are the 4-wave kernels.
// Refresh (RMU_OPT_SCREEN_REFRESH; spill launches only): at the start of every pair of tiles a wave used to read its queries' words from LDS (a
// load hipcc can see: its use waits lgkmcnt(0) and drains the four prefetched fragments right behind the ring barrier), raise thr_s, share it
// between the lane halves, and at step 4 issue the 4-byte LDS-DMA that fetches the words again.  A spilling wave cannot use any of it: the word
// is the one the last sift or merge published, only a compaction raises it, only a wave that fell back compacts, and the argument above never
// needed a wave to see a raise -- a wave that filters with an older, lower word spills a superset, the sift tests against the word as it stands
// after the launch, the merged keys and the next seeds are the same bits.  So a wave does that work only while `thr_live` holds: the launch is
// no spill launch, the wave has fallen back (it compacts and appends again: shared thresholds matter again; until its next DMA lands it reads
// the words of its first refresh -- older, lower, safe), it is at its first pair (the seeds arrive through this very path), it is the pacing
// wave (its DMA carries the siblings' progress words), or option 10 asks for it (ScanLaunch::share_thr bit 3: every wave, every pair, as it
// always was).  Dropping refreshes from a wave's VMEM stream only makes the ring's counted waits cover more.  Measured (profiles/
// screen_refresh.md): the pair prologue 350 -> 162 cycles per wave and pair in the debug build, the headline -0.08 .. -0.10 ms (1.3-1.5 %) in
// eight interleaved pairs of two records -- twice the span of the parent's legs in one record, short of it in the other; a third of what the
// prologue gives back is spent waiting at the pair barrier.  With option 10 = 1 this kernel is 0.9 % SLOWER than the one that had no branch
// there (the two scalar branches and what they do to the schedule around the barrier), so the default is 0.
// (An earlier hi/lo split variant, 3 MFMAs per 16 k with EPS = 1e-4, ran at 25 ms for the 10M x 1024 headline; its
// ablations showed the LDS/L2 path, not the MFMA pipe, setting the time, which is what halving the bytes attacks.)
#include <cstdlib>
#include <mutex>
#include <type_traits>
#include "rmu_common.h"
#include "scan_common.h"
#include "../../include/rmu.h"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// the pacing wave of the 8-wave kernels (see "sibling pacing" in scan_screen_lean3_kernel): 0..3, a compile-time constant so that builds with
// another wave can be set against each other under the debug counters (-DRMU_SCREEN_PW=n: profiles/screen_late_waves.md 2)
#ifndef RMU_SCREEN_PW
#define RMU_SCREEN_PW 0
#endif
static_assert(RMU_SCREEN_PW >= 0 && RMU_SCREEN_PW <= 3, "the pacing wave is the older wave of a SIMD");

namespace {

constexpr int SD = 384;                 // floats per row
constexpr int IMGB = RMU_IMG_ROW_BYTES; // 768: screening-image bytes per row
static_assert(IMGB == SD * 2, "image geometry");
constexpr int S_RT = 32;                // rows per tile (all waves of a workgroup share it)
constexpr int S_CKB = IMGB / 2;         // 384 B per row per chunk: a tile is streamed as two half-k chunks
constexpr int S_U16 = S_CKB / 16;       // 24 16-byte units per row per chunk
constexpr int S_TS = SD / 16;           // 24 MFMA steps per tile ...
constexpr int S_CS = S_TS / 2;          // ... 12 per chunk
constexpr int S_SLOT = S_RT * S_CKB;    // 12 KiB ring slot
extern __shared__ __attribute__((aligned(16))) char ssm[];

// EPS(q) of the header, in the one order both of its users take: |q|^2 and |dq|^2 run over k as the re-score kernel's chain does (step t holds
// k = 8t .. 8t+3 in qa and 8t+4 .. 8t+7 in qb, taken alternately), then the bound.  L2: the index stores 2q -- the query itself is half of it --
// and the norm's roundings add 1.5e-5 |x|max^2 (see k_rescore).  k_rescore tests with it; the query conversion computes the same number in
// front of the ladder for the band seeding of the merges (topk_merge.hip: seed_band).
template <bool L2>
__device__ __forceinline__ void screen_eps_step(const f32x4& qa, const f32x4& qb, float& qn2, float& dq2) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float ua = L2 ? 0.5f * qa[c] : qa[c], ub = L2 ? 0.5f * qb[c] : qb[c];      // the query itself (the L2 index stores 2q)
        qn2 = fmaf(ua, ua, qn2);
        qn2 = fmaf(ub, ub, qn2);
        const float da = ua - (float)(_Float16)(ua * 64.0f) * (1.0f / 64.0f);
        const float db = ub - (float)(_Float16)(ub * 64.0f) * (1.0f / 64.0f);
        dq2 = fmaf(da, da, dq2);
        dq2 = fmaf(db, db, dq2);
    }
}
template <bool L2>
__device__ __forceinline__ float screen_eps(float qn2, float dq2, float xnorm_max, float dx_max) {
    const float qn = sqrtf(qn2) * 1.0001f, dq = sqrtf(dq2) * 1.0001f;
    return dx_max * qn + xnorm_max * dq + dx_max * dq + 5.0e-5f * xnorm_max * qn +   // see the header
           (L2 ? 1.5e-5f * xnorm_max * xnorm_max : 0.f);
}

// fp32 rows [n, 384 of `stride` floats] -> screening image [n, 768 B] = fp16(scale * x); one thread per group of 8 k.  scale = 64, or 32 for the
// L2 index's queries, which are stored doubled (rmu_api.hip: k_l2_aug_queries)
// (round 6, second session) zero_a / zero_b: words the FIRST workgroup zeroes on the way -- the query conversion opens every screened search, and
// the ladder's shared thresholds and the re-run count used to be two memsets in front of it (~4.5 us of kernel boundary each)
// eps_out (optional, [n_eps]): EPS(q) of each of the n_eps rows of src, by the blocks from conv_blocks on -- a launch of its own would cost the same 4.5 us
__global__ void k_split_rows(const float* __restrict__ src, char* __restrict__ dst, int64_t n_groups, int stride, float scale,
                             u32* __restrict__ zero_a, int n_zero_a, u32* __restrict__ zero_b, int n_zero_b, int conv_blocks,
                             float* __restrict__ eps_out, int64_t n_eps, float xnorm_max, float dx_max, int l2) {
    if ((int)blockIdx.x >= conv_blocks) {       // the blocks behind the conversion: EPS(q) of the ladder's band seeding, one query per thread
        const int64_t qi = (int64_t)(blockIdx.x - conv_blocks) * blockDim.x + threadIdx.x;
        if (qi >= n_eps) return;
        const float* qv = src + qi * stride;
        float qn2 = 0.f, dq2 = 0.f;
#pragma unroll 4
        for (int t = 0; t < SD / 8; ++t) {
            const f32x4 qa = *(const f32x4*)(qv + 8 * t), qb = *(const f32x4*)(qv + 8 * t + 4);
            if (l2) screen_eps_step<true>(qa, qb, qn2, dq2);
            else screen_eps_step<false>(qa, qb, qn2, dq2);
        }
        eps_out[qi] = l2 ? screen_eps<true>(qn2, dq2, xnorm_max, dx_max) : screen_eps<false>(qn2, dq2, xnorm_max, dx_max);
        return;
    }
    if (blockIdx.x == 0) {
        for (int i = threadIdx.x; i < n_zero_a; i += blockDim.x) zero_a[i] = 0u;
        for (int i = threadIdx.x; i < n_zero_b; i += blockDim.x) zero_b[i] = 0u;
    }
    const int64_t gidx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gidx >= n_groups) return;
    const float* s = src + (gidx / (SD / 8)) * stride + (gidx % (SD / 8)) * 8;
    f16x8 hi;
#pragma unroll
    for (int e = 0; e < 8; ++e) hi[e] = (_Float16)(s[e] * scale);
    *(f16x8*)(dst + gidx * 16) = hi;
}

// err2[r] = |x_r - h_r / 64|^2: the measured rounding error of the screening image, one wave per row
__global__ __launch_bounds__(256) void k_img_err(const float* __restrict__ x, int64_t n, float* __restrict__ err2, int stride) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    const float* row = x + r * stride;
    float s = 0.f;
    for (int c = lane; c < SD; c += 64) {
        const float d = row[c] - (float)(_Float16)(row[c] * 64.0f) * (1.0f / 64.0f);
        s = fmaf(d, d, s);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) err2[r] = s * 1.0001f;   // summation slack
}

// ---- lean form, one barrier per TWO tiles (round 4): the screening kernel (the earlier forms are retired) ------------------------------
// Workgroup = NWV waves x 32 queries; every wave multiplies the same 32-row tiles by its own queries, whose fragments stay in registers for
// the whole scan: NWV = 4 with one v_mfma_f32_32x32x16_f16 per 16 k (24 per tile), NWV = 8 with v_mfma_f32_16x16x32_f16 -- a fragment is 16
// rows x 32 k and feeds two MFMAs back to back, queries 0-15 and 16-31 of the wave (48 per tile, the same 24 fragment reads, four f32x4
// accumulators).  Same cycles, same LDS bytes; the chip holds a higher clock on the smaller shape (tools/ubench/mfma_power.hip,
// profiles/mfma_shape.txt: 1.56 against 1.40 PFLOP/s for fragment stream + fill on random f16; profiles/screen_mfma_shape.md for the kernel).
// The 8-wave filter runs in the MFMA's own accumulator layout -- a lane holds 8 scores of each of two queries: a running maximum and one compare
// per query group -- and the accumulators change owner (eight v_permlane32_swap: to_owner) only when something passes.
// NWV = 8: full query tiles (256 queries per workgroup, batches over 128), TWO waves per SIMD.  A lone wave per SIMD issues roughly one
// instruction per 6-7 cycles in a wait / MFMA / ds_read / VALU mix (tools/ubench/mfma_issue.hip: 46 cycles per MFMA bare, 65 with five
// VALU fillers), which keeps the matrix pipe under half busy; two interleaved instruction streams hide each other's issue gaps.  (64
// queries per wave on 4 waves would feed two MFMAs per A fragment, but needs 192 registers of query fragments and ends issue-bound.)
// The limit is then the LDS return path: one 1-KiB A fragment per 32-cycle MFMA per SIMD is all of its 128 B/clk per CU.
// NWV = 4: ONE query tile (batches <= 128 queries): every image byte is read by exactly one workgroup -- NT streams it past the L2 with
// non-temporal loads.  The HBM-bound regime, where the instruction count per tile is what must stay small: one wave per SIMD has to issue
// them and keep 24 KiB per microsecond in flight.
// What a tile costs besides its 24 MFMAs ("32 cycles per MFMA + 6-11 per OTHER instruction of the wave" fit every form measured):
//   ring slots       the tile loop is unrolled over the ring's period (six bodies) so that every slot is a compile-time constant: fragment
//                    reads are ds_read_b128 with the slot folded into the 16-bit offset field, no address arithmetic
//   DMA pieces       LDS target = per-wave base + constant; source = ONE running 64-bit tile pointer + a per-lane 32-bit offset that already
//                    contains the piece's look-ahead of four tiles; no clamp -- the look-ahead past the last tile reads the image's slack
//                    rows (rmu_api.hip: kSlackRows, zero-filled) or the next chunk's rows, and is never consumed.  The pieces are issued one
//                    at a time between MFMA steps, not as a burst: a wave that cannot hand its VMEM instruction to the (busy) address unit
//                    cannot issue MFMAs either
//   filter           a running v_max3 over the previous tile's 16 scores (8 VALU) and ONE compare per tile; the per-lane work
//                    (slow_path) runs only when some lane passes
// Candidates live in GLOBAL memory (a.gcand: [chunk][query][CAP] keys, L2 resident), not in LDS: both lanes (j, j + 32) of a query
// belong to the one wave that filters it, so a slot's count is a REGISTER (equal in both lanes through one shuffle per append) and an append
// is a fire-and-forget store -- no LDS atomic, no wait.  Compaction (a full slot: rare once thresholds are seeded) and the emit read the slot
// back with sc1, past the vector L1.  That leaves the LDS to the ring: it holds SIX tiles (12 half-k slots, 144 KiB) and is handed over once
// per PAIR of tiles (a barrier per tile cost ~350 cycles of per-tile jitter); every wave carries 24 / NWV of a tile's 24 one-KiB DMA pieces.
// At the barrier of pair p the tiles up to 2p + 2 have landed (the fragment prefetch crosses into the next pair's first tile), 2p + 3 may be
// in flight, and pair p + 2 is issued during pair p into the slots of pair p - 1.
template <int NWV, bool DEEP = false>
struct Lean3Cfg {
    static constexpr int NW = NWV, QW = 32, NR = 12, NDW = NWV, NIW = 24 / NWV;
    // DEEP (round 6): 32 < k <= 104 -- K' <= 120 candidates per (chunk, query) slot of 128 keys, two keys per lane wherever the whole wave works
    // on one slot (compaction, emit); everything else -- ring, MFMA chain, filter, appends -- is the K' <= 40 kernel unchanged
    static constexpr int CAP = DEEP ? RMU_KS_CAP_DEEP : RMU_KS_CAP, NPL = DEEP ? 2 : 1;
    static constexpr int RING_BYTES = NR * S_SLOT;
    static constexpr int GT_OFF = RING_BYTES;
    static constexpr int NRM_OFF = GT_OFF + NW * 256;      // L2 form: -2048 |x|^2 of the rows of the six ring tiles (32 floats per tile)
    static constexpr int LDS_BYTES = NRM_OFF + 6 * S_RT * 4;
};

// L2N = 1 (round 5): the index ranks by 2 q.x - |x|^2 (RMU_METRIC_L2SQ).  The image has no k-slot left for the norm (384 fp16 = the 24 MFMA
// steps exactly), so it enters as the chain's C operand: a.nrm[row] = -2048 |x|^2 (fp32, built at add time from the exact scan's own
// -|x|^2 column) initialises the accumulator of the tile's first MFMA -- acc = 4096 (q~.x~ - |x|^2 / 2), the approximate HALF score; filter,
// thresholds, candidate keys and merges never know.  A lane's 16 accumulator rows (4h + 8i + c) are four 16-byte LDS reads (NWV = 8: its native
// rows 16 t + 4 (lane >> 4) + c are two, one per row half, shared by both query groups; the L2 instantiations run the 16x16x32 body too), issued half a
// tile ahead between two fragment reads (the lgkmcnt of the four steps behind them counts them in); the norms of a PAIR of tiles are one
// 256-byte LDS-DMA by wave 0, issued two pairs ahead next to the threshold refresh (older than the pieces the pair barrier's vmcnt leaves
// in flight, like the refresh).  +4 KiB-reads per 24 on the LDS return path; the fp16 image bytes are unchanged.
// EXP: bit 2 = cycle / event counters into a.dbg (debug builds, RMU_SCAN_EXP=7); bits 0, 1, 3 drop the corpus DMA, the fragment reads or the
// filter (timing ablations: wrong results by design)
template <int EXP = 0, int NWV = 8, int NT = 0, int L2N = 0, bool DEEP = false>
__global__ __launch_bounds__(64 * NWV) void scan_screen_lean3_kernel(const ScanLaunch a) {
    using C = Lean3Cfg<NWV, DEEP>;
    constexpr bool DBG = (EXP & 4) != 0;
    constexpr int NW = NWV, S_PRE = 4;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // Lane roles of the candidate path (filter slow path, appends, compaction, epilogue, emit): lane (h, j) owns query j of the wave and the
    // tile rows 4h + 8i + c (i, c = 0..3); the query's other lane is lane ^ XL.  NWV = 4 (32x32x16): that is the MFMA's own D layout, h = lane
    // bit 5.  NWV = 8 (16x16x32): the accumulators reach that ownership through to_owner() only when something passes; there h = lane bit 4
    // and j = 16 (lane bit 5) + (lane & 15).  qlane(jj): the h = 0 lane of query jj; jl: this lane's own one; qidx: the query of an h = 0 lane.
    constexpr bool M16 = NWV == 8;
    constexpr int XL = M16 ? 16 : 32;
    const int h = M16 ? (lane >> 4) & 1 : lane >> 5, j = M16 ? 16 * (lane >> 5) + (lane & 15) : lane & 31;
    const int jl = M16 ? lane & 47 : j;
    auto qlane = [](int jj) { return M16 ? 32 * (jj >> 4) + (jj & 15) : jj; };
    auto qidx = [](int ll) { return M16 ? 16 * (ll >> 5) + (ll & 15) : ll; };
    int s_idx, qt;   // row chunk, query tile
    block_map(a.s_chunks, a.nqt, s_idx, qt);
    const int64_t tiles_total = (a.n_rows + S_RT - 1) / S_RT;
    const int64_t t0 = (int64_t)s_idx * a.tiles_per_chunk;
    int64_t t1 = t0 + a.tiles_per_chunk;
    if (t1 > tiles_total) t1 = tiles_total;
    const int ntiles = (int)(t1 > t0 ? t1 - t0 : 0);
    const char* img = (const char*)a.x + a.row0 * (int64_t)IMGB;
    char* ring = ssm;
    const int q_base = (qt * NW + w) * C::QW;
    const bool q_ok = q_base + j < a.nq;
    const bool wave_live = q_base < a.nq;                 // (uniform)
    float thr_s = q_ok ? -INFINITY : INFINITY;            // 4096 * max(own k-th best, shared threshold): only ever rises
    u32 cnt = 0;                                          // entries in this lane's query slot (equal in lanes j and j + 32)
    u64* const gslot = a.gcand + ((size_t)s_idx * a.nq + (q_ok ? q_base + j : 0)) * C::CAP;
    u32* gthr_w = a.gthr + q_base;
    const u32* gt_lds = (const u32*)(ssm + C::GT_OFF) + w * 64;
    // ---- sibling pacing (2..4 query tiles, one workgroup per CU: rmu_screen_plan decides) ----------------------------------------------
    // The nqt workgroups that scan the SAME row chunk for different query tiles sit on one XCD (block map above) so that the chunk's image
    // bytes come from HBM once and from that XCD's L2 nqt - 1 times -- which only works while the siblings stay within an L2 window of each
    // other, and left alone they can drift (slow tiles, compactions: round 3 measured 1.97x the image in HBM fetches).  The whole grid is
    // resident at once, so the kernel lasts as long as its slowest workgroup and a leader that waits loses nothing.  Every workgroup
    // publishes ~tile (0 = not started / finished = "ignore me") once per pair of tiles, reads its siblings' words a pair stale through the
    // same 4-byte LDS-DMA that refreshes the shared thresholds (lanes 32..35: no extra VMEM instruction), and the pacing wave holds the
    // workgroup at the ring barrier while it is more than a.pace tiles ahead of the slowest sibling.  A HINT only: the wait is bounded (a
    // sibling that is not resident -- another kernel on the device -- switches pacing off for this workgroup).  The pacing wave (PW below)
    // publishes with a plain store issued a whole pair before its next counted ring wait: vmcnt retires in order, so a store that waits
    // for an agent-scope acknowledgement in front of those waits holds the ring up (the first version, an agent-scope store, doubled the
    // kernel's time).  The siblings share this XCD's L2, where the store lands, and read it with sc1 (past their vector L1).
    // Which wave paces (NWV = 8): one of the OLDER wave of each SIMD's two, 0..3.  Issue arbitration between the two is by age, so waves 0..3
    // reach the pair barrier long before waves 4..7 and wait there (profiles/screen_refresh.md 2: ~1 360 against ~240 cycles per pair);
    // the pacing wave's prologue -- threshold read and its lgkmcnt(0), update, progress store, the siblings' words and a second lgkmcnt(0)
    // -- was on wave 7, the wave everybody else waited for.  On an early wave it is paid out of that wave's slack
    // (profiles/screen_late_waves.md).  The 4-wave kernels never pace (rmu_screen_plan: 2..4 query tiles) and keep their constant.
    const bool pace_on = a.prog != nullptr;
    u32* prog_w = a.prog + (size_t)s_idx * 4;
    bool pace_live = pace_on;
    const u32* gsrc = gthr_w + (lane & 31);              // (LDS word l comes from lane l: word jj is query jj's threshold in either lane mapping)
    if (pace_on && lane >= 32 && lane < 36) gsrc = prog_w + (lane - 32);
    // (uniform) this wave still reads and refreshes its thresholds at every pair: see "Refresh" in the file header.  Set where a pair starts
    // (NWV = 8 only: the 4-wave kernels never assign it and compile as they did); the prologue's refresh carries the launch's seeds.
    int thr_live = 1;       // (an int: as a second bool beside pace_live the two end up in scratch, their stores sunk into one through a pointer)
    auto refresh_gthr = [&]() {
        if (!thr_live) return;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                         (__attribute__((address_space(3))) void*)(ssm + C::GT_OFF + w * 256), 4, 0, 16);
    };
    constexpr int PW = M16 ? RMU_SCREEN_PW : NW - 1;
    auto pace_step = [&](int tile) {
        if (lane == 0) __hip_atomic_store(prog_w + qt, ~(u32)tile, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        const u32 m4 = max(max(gt_lds[32], gt_lds[33]), max(gt_lds[34], gt_lds[35]));
        int lead = m4 ? tile - (int)~m4 : -1;
        if (__builtin_expect(__builtin_amdgcn_readfirstlane(lead) > a.pace, 0)) {
            int spins = 0;
            do {
                __builtin_amdgcn_s_sleep(24);
                u32 v = 0;
                if (lane < 4) v = __hip_atomic_load(prog_w + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                v = max(v, (u32)__shfl_xor((int)v, 1));
                v = max(v, (u32)__shfl_xor((int)v, 2));
                const u32 vm = (u32)__builtin_amdgcn_readfirstlane((int)v);
                lead = vm ? tile - (int)~vm : -1;
            } while (lead > a.pace && ++spins < 400);
            if (spins >= 400) pace_live = false;
        }
    };
    // NWV = 4: qh[T] = k-step T (16 k) of query j, k-half h.  NWV = 8: qh[12 g + s] = k-step s (32 k) of query 16 g + (lane & 15), k-group lane >> 4
    f16x8 qh[S_TS];
    if constexpr (M16) {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const int qi = q_base + 16 * g + (lane & 15);
            const char* qrow = (const char*)a.q + (size_t)(qi < a.nq ? qi : 0) * IMGB + (lane >> 4) * 16;
#pragma unroll
            for (int sk = 0; sk < S_TS / 2; ++sk) qh[12 * g + sk] = *(const f16x8*)(qrow + sk * 64);
        }
    } else {
        const char* qrow = (const char*)a.q + (size_t)(q_ok ? q_base + j : 0) * IMGB + h * 16;
#pragma unroll
        for (int T = 0; T < S_TS; ++T) qh[T] = *(const f16x8*)(qrow + T * 32);
    }
    {
#pragma unroll
        for (int T = 0; T < S_TS; ++T) asm volatile("" : "+v"(qh[T]));
        // The loads must be COMPLETE, as far as the compiler's wait-count pass can tell, before the first LDS-DMA is issued: it cannot count
        // through the ring's inline-asm waits, so a query fragment still "pending" at the loop head gets an s_waitcnt vmcnt(0) in front of its
        // first MFMA -- inside the loop, draining the DMA ring once per trip.
    }
    // DMA: wave w carries pieces n * NW + w (n = 0..NIW-1) of a tile's 24 = 12 * half + piece; issued during tile t they belong to tile t + 4.
    // Ring layout: a slot holds one half-k chunk of a tile, 32 rows x 384 B; LDS unit f -> row f / 24, and physical unit f % 24 of a row holds
    // logical unit p ^ ((row >> 1) & 7).  Rows are 384 B = 96 banks apart, so they alternate between two bank halves; the XOR spreads 8 row
    // pairs over the 8 units of an aligned block: any 16 consecutive rows reading one logical unit touch 16 distinct 4-bank groups (conflict free).
    u32 dma_off[C::NIW];
    int dma_dst[C::NIW];
#pragma unroll
    for (int n = 0; n < C::NIW; ++n) {
        const int id = n * C::NDW + w;
        const int half = id / 12, pid = id % 12;
        const int f = pid * 64 + lane;
        const int i = f / S_U16, p = f % S_U16;
        dma_off[n] = (u32)(i * IMGB + (p ^ ((i >> 1) & 7)) * 16 + half * S_CKB) + 4u * S_RT * IMGB;
        dma_dst[n] = half * S_SLOT + pid * 1024;
    }
    const char* tp = img + (t0 * S_RT) * (int64_t)IMGB;   // the current tile's rows (uniform)
    auto issue_part = [&](auto TS, const char* base, int n) {   // TS = ring position (0..5) of the tile the piece belongs to
        if (EXP & 1) return;
        if (NT)        // literal aux operands only
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(base + dma_off[n]),
                                             (__attribute__((address_space(3))) void*)(ring + decltype(TS)::value * 2 * S_SLOT + dma_dst[n]), 16, 0, 2);
        else
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(base + dma_off[n]),
                                             (__attribute__((address_space(3))) void*)(ring + decltype(TS)::value * 2 * S_SLOT + dma_dst[n]), 16, 0, 0);
    };
    // A fragment of (row j, chunk step t): logical unit 2t + h = 8 (t >> 2) + (2 (t & 3) + h); the XOR touches the low three bits only, so four
    // per-lane bases + an immediate (t >> 2) * 128 address a whole chunk.  Fragment reads and the waits on them are inline asm: left to itself
    // hipcc sinks every ds_read to just before the MFMA that consumes it and waits lgkmcnt(0) there (a 32-cycle MFMA cannot hide an LDS round
    // trip).  The reads keep their program order (volatile), S_PRE of them are in flight, and frag_wait ties the counted wait to the register
    // the MFMA reads, so the MFMA cannot be scheduled above it.
    // NWV = 8: a fragment is 16 rows x 32 k -- lane l reads row 16 t + (l & 15) (t = row half), logical unit 4 T' + (l >> 4) of the chunk
    // (T' = 0..5): TWO per-lane bases (T' & 1) + immediates t * 6144 + (T' >> 1) * 128 (rows 16 apart share the XOR: (16 >> 1) & 7 = 0).
    // Conflict free under the same swizzle (tests/test_screen_shape_cpu.py).  Read index i = 0..11 of a chunk is (T' = i >> 1, t = i & 1).
    constexpr int NAB = M16 ? 2 : 4;
    u32 ab[NAB], ab_hi[NAB], ab_h2[NAB];                  // (the offset field is 16 bits: slots 4..7 and 8..11 go through their own bases)
#pragma unroll
    for (int m = 0; m < NAB; ++m) {
        if constexpr (M16) ab[m] = lds_addr(ring) + (u32)((lane & 15) * S_CKB + (((4 * m + (lane >> 4)) ^ (((lane & 15) >> 1) & 7)) * 16));
        else ab[m] = lds_addr(ring) + (u32)(j * S_CKB + (((2 * m + h) ^ ((j >> 1) & 7)) * 16));
        ab_hi[m] = ab[m] + 4u * S_SLOT;
        ab_h2[m] = ab[m] + 8u * S_SLOT;
    }
    f16x8 fr[S_PRE];
#pragma unroll
    for (int m = 0; m < S_PRE; ++m) fr[m] = f16x8{};
    auto read_frag = [&](f16x8& dst, auto OFF, int t) {   // t: which per-lane base
        if (EXP & 2) { asm volatile("" : "+v"(dst)); return; }
        constexpr int off = decltype(OFF)::value;
        const u32 ad = off >= 8 * S_SLOT ? ab_h2[t & (NAB - 1)] : off >= 4 * S_SLOT ? ab_hi[t & (NAB - 1)] : ab[t & (NAB - 1)];
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(ad), "n"(off % (4 * S_SLOT)));
    };
    auto frag_wait = [&](f16x8& f) {
        if (EXP & 2) return;
        asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(f) : "n"(S_PRE - 1));
    };
    auto frag_wait_nrm = [&](f16x8& f) {                   // the four (NWV = 8: two) norm reads sit between this fragment's read and the newest ones
        if (EXP & 2) return;
        if constexpr (M16) asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(f) : "n"(S_PRE - 1 + 2));
        else asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(f) : "n"(S_PRE - 1 + 4));
    };
    // L2 form: row norms of the ring tiles
    const float* np = L2N ? a.nrm + a.row0 + t0 * S_RT + lane : nullptr;     // one float per lane = the 64 rows of a pair of tiles
    const u32 nrm_ad = lds_addr(ssm + C::NRM_OFF) + (u32)(M16 ? lane >> 4 : h) * 16u;
    f32x4 zq[4] = {};
    auto issue_nrm = [&](auto PI, const float* src) {      // PI = ring position of the pair's first tile
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(ssm + C::NRM_OFF + decltype(PI)::value * S_RT * 4), 4, 0, 0);
    };
    auto read_nrm = [&](auto PI) {                         // this lane's 16 accumulator rows of the tile at ring position PI: rows 4h + 8i + (0..3)
        constexpr int o = decltype(PI)::value * S_RT * 4;
        f32x4 &z0 = zq[0], &z1 = zq[1], &z2 = zq[2], &z3 = zq[3];      // (asm operands alone do not capture in a generic lambda)
        const u32 ad = nrm_ad;
        if constexpr (M16) {                               // native rows 16 t + 4 (lane >> 4) + c: one read per row half, the same for both query groups
            asm volatile("ds_read_b128 %0, %2 offset:%3\n\tds_read_b128 %1, %2 offset:%4" : "=v"(z0), "=v"(z1) : "v"(ad), "n"(o), "n"(o + 64));
            return;
        }
        asm volatile("ds_read_b128 %0, %4 offset:%5\n\tds_read_b128 %1, %4 offset:%6\n\tds_read_b128 %2, %4 offset:%7\n\tds_read_b128 %3, %4 offset:%8"
                     : "=v"(z0), "=v"(z1), "=v"(z2), "=v"(z3)
                     : "v"(ad), "n"(o), "n"(o + 32), "n"(o + 64), "n"(o + 96));
    };
    u32 d_slow = 0, d_comp = 0, d_app = 0;
    unsigned long long d_clk_slow = 0, d_clk_bar = 0, d_clk_vm = 0, d_clk_pro = 0, d_clk_all = DBG ? clock64() : 0;
    // keep the best K' of query lane jj's slot (sorted), raise its threshold, publish it.  Every VMEM operation of compact and slow_path is
    // inline asm: one the compiler can see puts an s_waitcnt vmcnt(0) in front of the tile loop's first MFMA -- the join of this path -- and
    // drains the DMA ring once per tile.
    auto compact = [&](int jj) {                           // jj: the query's h = 0 lane
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const u32 n = (u32)__builtin_amdgcn_readlane((int)cnt, jj);
        u64* slot = (u64*)(((u64)(u32)__builtin_amdgcn_readlane((int)(u32)((u64)gslot >> 32), jj) << 32) |
                           (u64)(u32)__builtin_amdgcn_readlane((int)(u32)(u64)gslot, jj));
        u64 key[C::NPL];
        u32 rank[C::NPL];
#pragma unroll
        for (int pp = 0; pp < C::NPL; ++pp) {
            key[pp] = 0ull;
            if ((u32)(lane + 64 * pp) < n) asm volatile("global_load_dwordx2 %0, %1, off sc1" : "=v"(key[pp]) : "v"(slot + lane + 64 * pp) : "memory");
        }
#pragma unroll
        for (int pp = 0; pp < C::NPL; ++pp) asm volatile("s_waitcnt vmcnt(0)" : "+v"(key[pp])::"memory");
        rank_keys<C::NPL>(key, n, rank);
#pragma unroll
        for (int pp = 0; pp < C::NPL; ++pp) {
            const bool keep = (u32)(lane + 64 * pp) < n && rank[pp] < (u32)a.k;
            if (keep) asm volatile("global_store_dwordx2 %0, %1, off" ::"v"(slot + rank[pp]), "v"(key[pp]) : "memory");
            const u64 kb = __ballot(keep && rank[pp] == (u32)(a.k - 1));
            if (kb) {
                const u32 hi = (u32)__builtin_amdgcn_readlane((int)(u32)(key[pp] >> 32), __builtin_ctzll(kb));
                if (jl == jj) thr_s = fmaxf(thr_s, rmu_ord2f(hi) * 4096.0f);
                if (lane == 0) asm volatile("global_atomic_umax %0, %1, off sc1" ::"v"(gthr_w + qidx(jj)), "v"(hi) : "memory");
            }
        }
        if (jl == jj) cnt = n < (u32)a.k ? n : (u32)a.k;
        if (DBG) ++d_comp;
    };
    auto slow_path = [&](const f32x16& p, int64_t rbase, u32 inmask) __attribute__((always_inline)) {   // (out of line it would put the kernel's state into scratch)
        unsigned long long c0 = 0;
        u32 todo = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) todo |= (p[r] > thr_s) ? (1u << r) : 0u;
        todo &= inmask;
        if (DBG) { ++d_slow; d_app += __builtin_popcount(todo); c0 = clock64(); }
        u32 uni = 0;
        for (u64 bl = __ballot(todo != 0); bl; bl &= bl - 1) uni |= (u32)__builtin_amdgcn_readlane((int)todo, __builtin_ctzll(bl));
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if ((uni >> r) & 1u) {
                bool has = ((todo >> r) & 1u) && p[r] > thr_s;
                u32 other = (u32)__shfl_xor((int)has, XL);
                const u64 full = __ballot(cnt + (u32)has + other > (u32)C::CAP);
                if (__builtin_expect(full != 0, 0)) {          // (both lanes of a query vote alike: its h = 0 lane stands for it)
                    if constexpr (M16) {
                        for (u64 fm = full & 0x0000ffff0000ffffull; fm; fm &= fm - 1) compact(__builtin_ctzll(fm));
                    } else {
                        for (u32 fm = (u32)full | (u32)(full >> 32); fm; fm &= fm - 1) compact(__builtin_ctz(fm));
                    }
                    has = has && p[r] > thr_s;
                    other = (u32)__shfl_xor((int)has, XL);
                }
                const u32 pos = cnt + (h ? other : 0u);
                if (has) {
                    const u64 key = rmu_make_key(p[r] * (1.0f / 4096.0f) + 0.0f, (u32)(rbase + (r & 3) + 8 * (r >> 2)));
                    asm volatile("global_store_dwordx2 %0, %1, off" ::"v"(gslot + pos), "v"(key) : "memory");
                }
                cnt += (u32)has + other;
            }
        }
        if (DBG) d_clk_slow += clock64() - c0;
    };
    // NWV = 8: the 16x16x32 accumulators in the MFMA's own layout, element 8 g + 4 t + c of a tile's f32x16 = query 16 g + (lane & 15), row
    // 16 t + 4 (lane >> 4) + c.  The fast filter works on it as it is: a running maximum per query group against that group's threshold (thr_g0 /
    // thr_g1: the threshold of query (lane & 15) and of query 16 + (lane & 15), whichever lane half owns it).  to_owner: eight half-swaps -- lanes
    // 32..63 of group 0's register against lanes 0..31 of group 1's -- leave lane 32 b5 + 16 b4 + n with query 16 b5 + n alone, rows 4 b4 + 8 i + c
    // at element 4 i + c, i = 2 t + (the register's old lane bit 5): slow_path's layout.
    float thr_g0 = thr_s, thr_g1 = thr_s;
    auto share_thr16 = [&]() {
        if constexpr (M16) {
            const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(thr_s), __float_as_uint(thr_s), false, false);
            thr_g0 = __uint_as_float(r[0]);
            thr_g1 = __uint_as_float(r[1]);
        }
    };
    share_thr16();
    auto to_owner = [&](const f32x16& nat) -> f32x16 {
        f32x16 p = nat;
        if constexpr (M16)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float g0 = nat[4 * t + c], g1 = nat[8 + 4 * t + c];      // (scalars first: a bit cast applied to a vector element reads element 0)
                const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(g0), __float_as_uint(g1), false, false);
                p[8 * t + c] = __uint_as_float(r[0]);
                p[8 * t + 4 + c] = __uint_as_float(r[1]);
            }
        return p;
    };
    // ---- spill path (NWV = 8, seeded launches: a.spill; see the file header) ---------------------------------------------------------------
    // A lane whose running maximum beats its group's threshold stores the 8 scores it holds of that group, as the MFMA left them, and
    // {tile, lane | group << 8} behind them: three 16-byte stores into the list of this (row chunk, query tile, wave).  The fill count is a
    // wave-uniform register, a lane's place is the count + its rank in the two ballots: no owner change, no walk over rows, no exchange with a
    // partner lane, no per-query count, no atomic and no wait.  Inline asm like every store of this path (a store hipcc can see costs the
    // tile loop an s_waitcnt vmcnt(0)); the s_nop 1 covers the data registers of a store wider than 64 bits (NOTES_r06.md 8).  A tile that
    // does not fit ends the wave's spilling: it and every later one take slow_path, whose slots are then emitted as ever (RMU_SPILL_FELL).
    typedef u32 u32x4 __attribute__((ext_vector_type(4)));
    const bool spill_launch = M16 && a.spill != nullptr;  // (uniform over the grid)
    const int sp_list = (s_idx * a.nqt + qt) * NW + w;    // (uniform)
    char* const sp_base = a.spill + (size_t)sp_list * (size_t)a.spill_cap * RMU_SPILL_REC;
    u32 sp_cnt = 0, d_spill = 0;                          // (uniform)
    bool sp_live = spill_launch;                          // (uniform) still spilling
    auto spill_tile = [&](const f32x16& nat, int tile, bool p0, bool p1) -> bool {
        const u64 b0 = __ballot(p0), b1 = __ballot(p1);
        const u32 n0 = (u32)__builtin_popcountll(b0), n1 = (u32)__builtin_popcountll(b1);
        if (sp_cnt + n0 + n1 > (u32)a.spill_cap) { sp_live = false; return false; }
        unsigned long long c0 = 0;
        if (DBG) { ++d_spill; c0 = clock64(); }
        const u32 r0 = sp_cnt + __builtin_amdgcn_mbcnt_hi((u32)(b0 >> 32), __builtin_amdgcn_mbcnt_lo((u32)b0, 0u));
        const u32 r1 = sp_cnt + n0 + __builtin_amdgcn_mbcnt_hi((u32)(b1 >> 32), __builtin_amdgcn_mbcnt_lo((u32)b1, 0u));
        if (p0) {
            const f32x4 v0 = {nat[0], nat[1], nat[2], nat[3]}, v1 = {nat[4], nat[5], nat[6], nat[7]};
            const u32x4 hd = {(u32)tile, (u32)lane, 0u, 0u};
            asm volatile("global_store_dwordx4 %0, %1, off\n\tglobal_store_dwordx4 %0, %2, off offset:16\n\tglobal_store_dwordx4 %0, %3, off offset:32\n\ts_nop 1"
                         ::"v"(sp_base + (size_t)r0 * RMU_SPILL_REC), "v"(v0), "v"(v1), "v"(hd) : "memory");
        }
        if (p1) {
            const f32x4 v0 = {nat[8], nat[9], nat[10], nat[11]}, v1 = {nat[12], nat[13], nat[14], nat[15]};
            const u32x4 hd = {(u32)tile, (u32)lane | 256u, 0u, 0u};
            asm volatile("global_store_dwordx4 %0, %1, off\n\tglobal_store_dwordx4 %0, %2, off offset:16\n\tglobal_store_dwordx4 %0, %3, off offset:32\n\ts_nop 1"
                         ::"v"(sp_base + (size_t)r1 * RMU_SPILL_REC), "v"(v0), "v"(v1), "v"(hd) : "memory");
        }
        sp_cnt += n0 + n1;
        if (DBG) d_clk_slow += clock64() - c0;
        return true;
    };
    using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>; using I3 = std::integral_constant<int, 3>;
    using I4 = std::integral_constant<int, 4>; using I5 = std::integral_constant<int, 5>;
    bool direct = false;      // (uniform per wave) this wave's lists are already in a.partial: see the cold tile below
    if (ntiles > 0) {
        refresh_gthr();
        if (L2N) {                                        // (older than every piece: complete at the first counted wait)
            if (w == 0) {
                issue_nrm(I0{}, np);
                issue_nrm(I2{}, np + 2 * S_RT);
            }
            np += 4 * S_RT;
        }
        {
            const char* b0 = tp - 4 * S_RT * IMGB;        // dma_off carries the in-loop look-ahead of four tiles
#pragma unroll
            for (int n = 0; n < C::NIW; ++n) issue_part(I0{}, b0, n);
#pragma unroll
            for (int n = 0; n < C::NIW; ++n) issue_part(I1{}, b0 + S_RT * IMGB, n);
#pragma unroll
            for (int n = 0; n < C::NIW; ++n) issue_part(I2{}, b0 + 2 * S_RT * IMGB, n);
#pragma unroll
            for (int n = 0; n < C::NIW; ++n) issue_part(I3{}, b0 + 3 * S_RT * IMGB, n);
        }
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(C::NIW) : "memory");   // tiles 0, 1, 2 (and the thresholds)
        __builtin_amdgcn_s_barrier();
        if (L2N && (NWV == 8 || wave_live)) read_nrm(I0{});   // (in front of the fragment prefetch: step 0's counted wait covers it)
        if constexpr (M16) {                               // reads 0..3 of tile 0's first chunk
            read_frag(fr[0], std::integral_constant<int, 0>{}, 0);
            read_frag(fr[1], std::integral_constant<int, 16 * S_CKB>{}, 0);
            read_frag(fr[2], std::integral_constant<int, 0>{}, 1);
            read_frag(fr[3], std::integral_constant<int, 16 * S_CKB>{}, 1);
        } else {
#pragma unroll
        for (int m = 0; m < S_PRE; ++m) {
            if (!(EXP & 2)) asm volatile("ds_read_b128 %0, %1" : "=v"(fr[m]) : "v"(ab[m]));
        }
        }
        f32x16 accA, accB;
#pragma unroll
        for (int r = 0; r < 16; ++r) { accB[r] = -INFINITY; accA[r] = 0.f; }
        const int64_t lane_r0 = a.row0 + t0 * S_RT + 4 * h;
        // one tile; P = its position in the six-tile ring (compile time): its chunks sit in slots 2P and 2P + 1
        auto tile_body = [&](auto PI, f32x16& acc, const f32x16& prev, int tl) {
            constexpr int P = decltype(PI)::value;
            unsigned long long cp = 0;                     // (debug counters) the pair barrier's release: d_clk_pro runs from here to step 0's wait
            if (P % 2 == 0) {                              // a pair of tiles starts
                unsigned long long cb = 0;
                if (DBG) cb = clock64();
                // in flight at most: the NIW pieces (tile tl + 3) this wave issued during the previous tile; the refresh is older
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(C::NIW) : "memory");
                if (DBG) { const unsigned long long cv = clock64(); d_clk_vm += cv - cb; cb = cv; }
                __builtin_amdgcn_s_barrier();              // tiles up to tl + 2 have landed; nobody reads the previous pair any more
                if (DBG) { cp = clock64(); d_clk_bar += cp - cb; }
                // A spill launch's thresholds are the words its seeds left: only a compaction raises one, only a wave that fell back compacts,
                // and the sift tests every spilled score against the final word.  Such a wave re-reads nothing from its second pair on (the
                // pacing wave goes on: its refresh carries the siblings' progress words).  A wave that falls back reads again from its next
                // pair on -- until its next refresh lands, the words of its first one: older, lower, a superset passes.
                if constexpr (M16) thr_live = (!sp_live || tl == 0 || (a.share_thr & 8) != 0 || (w == PW && pace_live)) ? 1 : 0;
                if (thr_live) {
                    const u32 go = gt_lds[j];
                    if (go && (a.share_thr & 1)) thr_s = fmaxf(thr_s, rmu_ord2f(go - 1u) * 4096.0f);
                    share_thr16();
                }
                if (w == PW && pace_live) pace_step(tl);
            }
            // (Measured per wave: waves 0-3 wait ~600 cycles per tile at the pair barrier, waves 4-7 ~75 -- issue arbitration between the two waves
            // of a SIMD is by age.  Giving the younger half s_setprio 1 for the first tile of every pair halves the total wait and changes
            // the kernel's time by nothing: the SIMD's throughput, not the rendezvous, sets it.)
            float mx = -INFINITY, mx1 = -INFINITY;
            // NWV = 8: one step = one counted wait, one ds_read_b128 and TWO v_mfma_f32_16x16x32_f16 -- the fragment (rows 16 t .., 32 k) times query
            // group 0 and group 1; read i of chunk cch is k-step 6 cch + (i >> 1) of row half t = i & 1, so each of the four accumulators
            // acc[g][t] is touched every fourth MFMA.  12 fp32 accumulations per score (inside the header's 408 * 2^-24).
            auto step16 = [&](auto TI) {
                constexpr int gs = decltype(TI)::value, i = gs % S_CS, cch = gs / S_CS;
                constexpr int cur = 2 * P + cch, nxt = (cur + 1) % C::NR;
                constexpr int tt = i & 1, sk = 6 * cch + (i >> 1), e0 = 4 * tt, e1 = 8 + 4 * tt;
                if (gs == 18 && !(a.share_thr & 2) && !(EXP & 8) && __builtin_expect(__ballot(mx > thr_g0 || mx1 > thr_g1) != 0, 0)) {
                    if (!(sp_live && spill_tile(prev, tl - 1, mx > thr_g0, mx1 > thr_g1))) {
                        slow_path(to_owner(prev), lane_r0 + (int64_t)(tl - 1) * S_RT, 0xffffu);
                        share_thr16();
                    }
                }
                if (L2N && gs >= 13 && gs <= 16) frag_wait_nrm(fr[gs % S_PRE]);
                else frag_wait(fr[gs % S_PRE]);
                if (DBG && gs == 0 && P % 2 == 0) d_clk_pro += clock64() - cp;   // the pair prologue: threshold read, update, share, pacing
                f32x4 c0, c1;
                if (sk == 0) {
                    c0 = L2N ? zq[tt] : f32x4{0.f, 0.f, 0.f, 0.f};
                    c1 = c0;
                } else {
                    c0 = f32x4{acc[e0], acc[e0 + 1], acc[e0 + 2], acc[e0 + 3]};
                    c1 = f32x4{acc[e1], acc[e1 + 1], acc[e1 + 2], acc[e1 + 3]};
                }
                c0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(fr[gs % S_PRE], qh[sk], c0, 0, 0, 0);
                c1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(fr[gs % S_PRE], qh[12 + sk], c1, 0, 0, 0);
#pragma unroll
                for (int c = 0; c < 4; ++c) { acc[e0 + c] = c0[c]; acc[e1 + c] = c1[c]; }
                if (gs >= 1 && gs <= 4 && !(EXP & 8)) asm("v_max3_f32 %0, %0, %1, %2" : "+v"(mx) : "v"(prev[2 * gs - 2]), "v"(prev[2 * gs - 1]));
                if (gs >= 5 && gs <= 8 && !(EXP & 8)) asm("v_max3_f32 %0, %0, %1, %2" : "+v"(mx1) : "v"(prev[2 * gs - 2]), "v"(prev[2 * gs - 1]));
                constexpr int ni = i + S_PRE < S_CS ? i + S_PRE : i + S_PRE - S_CS, ns = i + S_PRE < S_CS ? cur : nxt;
                read_frag(fr[gs % S_PRE], std::integral_constant<int, ns * S_SLOT + (ni & 1) * 16 * S_CKB + (ni >> 2) * 128>{}, ni >> 1);
                if (L2N && gs == 12) read_nrm(std::integral_constant<int, (P + 1) % 6>{});        // the NEXT tile's norms (landed: see the kernel's header)
                if (gs % (S_TS / C::NIW) == 1) issue_part(std::integral_constant<int, (P + 4) % 6>{}, tp, gs / (S_TS / C::NIW));   // steps 1, 9, 17
                if (gs == 4 && P % 2 == 0) refresh_gthr();
                if (L2N && gs == 4 && P % 2 == 0) {       // norms of the pair two pairs ahead, into the slots of the pair that has just been left
                    if (w == 0) issue_nrm(std::integral_constant<int, (P + 4) % 6>{}, np);
                    np += 2 * S_RT;
                }
                __builtin_amdgcn_sched_barrier(0);
            };
            auto step = [&](auto TI) {
                if constexpr (M16) {
                    step16(TI);
                } else {
                constexpr int gs = decltype(TI)::value, t = gs % S_CS, cch = gs / S_CS;
                constexpr int cur = 2 * P + cch, nxt = (cur + 1) % C::NR;
                // (a wave none of whose 32 queries exist -- batches below 97 queries in the one-tile form -- only carries its DMA pieces)
                if (NWV == 8 || wave_live) {
                if (gs == 18 && !(a.share_thr & 2) && !(EXP & 8) && __builtin_expect(__ballot(mx > thr_s) != 0, 0))
                    slow_path(prev, lane_r0 + (int64_t)(tl - 1) * S_RT, 0xffffu);
                if (L2N && gs >= 13 && gs <= 16) frag_wait_nrm(fr[gs % S_PRE]);
                else frag_wait(fr[gs % S_PRE]);
                if (gs == 0 && L2N) {
                    const f32x16 z = {zq[0][0], zq[0][1], zq[0][2], zq[0][3], zq[1][0], zq[1][1], zq[1][2], zq[1][3],
                                      zq[2][0], zq[2][1], zq[2][2], zq[2][3], zq[3][0], zq[3][1], zq[3][2], zq[3][3]};
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(fr[gs % S_PRE], qh[gs], z, 0, 0, 0);
                } else if (gs == 0) {
                    const f32x16 z = {};
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(fr[gs % S_PRE], qh[gs], z, 0, 0, 0);
                } else {
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(fr[gs % S_PRE], qh[gs], acc, 0, 0, 0);
                }
                // (the MFMAs as inline asm with the wait in the same statement -- no compiler s_nop padding -- measured no faster: 6.64-6.67 vs 6.54)
                if (gs >= 1 && gs <= 8 && !(EXP & 8)) asm("v_max3_f32 %0, %0, %1, %2" : "+v"(mx) : "v"(prev[2 * gs - 2]), "v"(prev[2 * gs - 1]));
                if (t + S_PRE < S_CS) read_frag(fr[gs % S_PRE], std::integral_constant<int, cur * S_SLOT + ((t + S_PRE) >> 2) * 128>{}, t + S_PRE);
                else read_frag(fr[gs % S_PRE], std::integral_constant<int, nxt * S_SLOT + ((t + S_PRE - S_CS) >> 2) * 128>{}, t + S_PRE - S_CS);
                if (L2N && gs == 12) read_nrm(std::integral_constant<int, (P + 1) % 6>{});        // the NEXT tile's norms (landed: see the kernel's header)
                }
                if (gs % (S_TS / C::NIW) == 1) issue_part(std::integral_constant<int, (P + 4) % 6>{}, tp, gs / (S_TS / C::NIW));   // steps 1, 9, 17 | 1, 5, .., 21
                if (gs == 4 && P % 2 == 0) refresh_gthr();
                if (L2N && gs == 4 && P % 2 == 0) {       // norms of the pair two pairs ahead, into the slots of the pair that has just been left
                    if (w == 0) issue_nrm(std::integral_constant<int, (P + 4) % 6>{}, np);
                    np += 2 * S_RT;
                }
                __builtin_amdgcn_sched_barrier(0);
                }
            };
            step(std::integral_constant<int, 0>{}); step(std::integral_constant<int, 1>{}); step(std::integral_constant<int, 2>{});
            step(std::integral_constant<int, 3>{}); step(std::integral_constant<int, 4>{}); step(std::integral_constant<int, 5>{});
            step(std::integral_constant<int, 6>{}); step(std::integral_constant<int, 7>{}); step(std::integral_constant<int, 8>{});
            step(std::integral_constant<int, 9>{}); step(std::integral_constant<int, 10>{}); step(std::integral_constant<int, 11>{});
            step(std::integral_constant<int, 12>{}); step(std::integral_constant<int, 13>{}); step(std::integral_constant<int, 14>{});
            step(std::integral_constant<int, 15>{}); step(std::integral_constant<int, 16>{}); step(std::integral_constant<int, 17>{});
            step(std::integral_constant<int, 18>{}); step(std::integral_constant<int, 19>{}); step(std::integral_constant<int, 20>{});
            step(std::integral_constant<int, 21>{}); step(std::integral_constant<int, 22>{}); step(std::integral_constant<int, 23>{});
            tp += S_RT * IMGB;
        };
        // ring period: six bodies (the accumulator parity alternates with it)
        if constexpr (M16) {
            // NWV = 8: whole periods run their six bodies unconditionally.  With every body behind `if (tl + i < ntiles)` the odd tiles'
            // accumulators were a phi of "body ran" and "body skipped", resolved by a 16-register copy (and the s_nop 5 that lets the last
            // MFMA's result be read) at every merge point right in front of the pair barrier, plus a scalar compare and branch per tile.
            // Here the two sets alternate in place; the last, partial period takes the conditional form, once per chunk.
            int tl = 0;
            for (; tl + 6 <= ntiles; tl += 6) {
                tile_body(I0{}, accA, accB, tl);
                tile_body(I1{}, accB, accA, tl + 1);
                tile_body(I2{}, accA, accB, tl + 2);
                tile_body(I3{}, accB, accA, tl + 3);
                tile_body(I4{}, accA, accB, tl + 4);
                tile_body(I5{}, accB, accA, tl + 5);
            }
            if (tl < ntiles) {                             // the remainder: one to five tiles
                tile_body(I0{}, accA, accB, tl);
                if (tl + 1 < ntiles) tile_body(I1{}, accB, accA, tl + 1);
                if (tl + 2 < ntiles) tile_body(I2{}, accA, accB, tl + 2);
                if (tl + 3 < ntiles) tile_body(I3{}, accB, accA, tl + 3);
                if (tl + 4 < ntiles) tile_body(I4{}, accA, accB, tl + 4);
            }
        } else {
        for (int tl = 0; tl < ntiles; tl += 6) {           // (NWV = 4: every period in the conditional form, as it was)
            tile_body(I0{}, accA, accB, tl);                 // (tile -1 = the -inf accumulators: nothing passes)
            if (tl + 1 < ntiles) tile_body(I1{}, accB, accA, tl + 1);
            if (tl + 2 < ntiles) tile_body(I2{}, accA, accB, tl + 2);
            if (tl + 3 < ntiles) tile_body(I3{}, accB, accA, tl + 3);
            if (tl + 4 < ntiles) tile_body(I4{}, accA, accB, tl + 4);
            if (tl + 5 < ntiles) tile_body(I5{}, accB, accA, tl + 5);
        }
        }
        if (pace_on && w == PW && lane == 0) __hip_atomic_store(prog_w + qt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int m = 0; m < S_PRE; ++m) asm volatile("" : "+v"(fr[m]));
        // (NWV = 8, L2 form) the same for the norms the last body read ahead: in the remainder period the compiler can see that nobody uses
        // them, and a dead output of an asm ds_read is a register it hands to something else while the LDS data is still on its way
        if constexpr (M16 && L2N != 0) asm volatile("" : "+v"(zq[0]), "+v"(zq[1]));
        {
            const bool last_in_a = ((ntiles - 1) & 1) == 0;
            f32x16 last;
            const int64_t rbl = lane_r0 + (int64_t)(ntiles - 1) * S_RT, row_end = a.row0 + a.n_rows;
            u32 inmask = 0;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                last[r] = last_in_a ? accA[r] : accB[r];
                inmask |= (rbl + (r & 3) + 8 * (r >> 2) < row_end) ? (1u << r) : 0u;
            }
            // spill launch: the last tile of the chunk is spilled like the others (rows past the range's end are dropped by the sift)
            bool last_spilled = false;
            if constexpr (M16) {
                if (sp_live && !(a.share_thr & 2)) {
                    float m0 = last[0], m1 = last[8];
#pragma unroll
                    for (int r = 1; r < 8; ++r) { m0 = fmaxf(m0, last[r]); m1 = fmaxf(m1, last[8 + r]); }
                    const bool p0 = m0 > thr_g0, p1 = m1 > thr_g1;
                    last_spilled = __ballot(p0 || p1) == 0ull || spill_tile(last, ntiles - 1, p0, p1);
                }
                last = to_owner(last);
            }
            // (round 6, second session) COLD tile of the ladder's first launch -- one tile per chunk, empty thresholds: every row of the tile is a
            // candidate of every query.  Through slow_path that is 16 store instructions of 64 scattered 8-byte keys per wave (the slots are
            // query-major, a query's lanes 384 B apart: every lane its own line request -- 112 k of a wave's 174 k cycles in the debug build), a
            // read-back and a copy.  Here the wave's 32 x 32 keys go through 8 KiB of the (now idle) ring and straight into a.partial, a store
            // instruction = two queries' lists = 512 contiguous bytes; the slots are never touched and the emit skips this wave.  The lists leave
            // unsorted (share_thr bit 2: the launch's merge knows).  The barrier is workgroup-uniform (share_thr, ntiles); `cold` is per wave.
            bool cold = false;
            if ((a.share_thr & 4) && !(a.share_thr & 2) && ntiles == 1 && a.k >= 32) {
                __builtin_amdgcn_s_barrier();            // every wave's DMA has landed (the drain above) and nobody reads the ring any more
                u32 todo = 0;
#pragma unroll
                for (int r = 0; r < 16; ++r) todo |= (last[r] > thr_s) ? (1u << r) : 0u;
                todo &= inmask;
                cold = __ballot(q_ok && (cnt != 0u || todo != 0xffffu)) == 0ull;
            }
            if (cold) {
                u64* tl = (u64*)(ring + w * 8192);       // [query 0..31][position 0..31]: lane (j, h) owns positions [16 h, +16) of query j
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    tl[j * 32 + 16 * h + r] = rmu_make_key(last[r] * (1.0f / 4096.0f) + 0.0f, (u32)(rbl + (r & 3) + 8 * (r >> 2)));
                __builtin_amdgcn_wave_barrier();
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                u64* const pbase = a.partial + ((size_t)s_idx * a.nq + q_base) * a.k;
#pragma unroll
                for (int it = 0; it < 16; ++it) {
                    const int lin = it * 64 + lane, qq = lin >> 5, pos = lin & 31;
                    const u64 key = tl[lin];
                    if (q_base + qq < a.nq) pbase[(size_t)qq * a.k + pos] = key;
                }
                const int extra = a.k - 32;                // positions 32 .. K' - 1 of every list: zeros
                for (int e = lane; e < 32 * extra; e += 64) {
                    const int qq = e / extra, pos = 32 + e % extra;
                    if (q_base + qq < a.nq) pbase[(size_t)qq * a.k + pos] = 0ull;
                }
                direct = true;
            } else if (!(a.share_thr & 2) && !last_spilled) slow_path(last, rbl, inmask);
        }
    }
    if (DBG) {
        u32 app = d_app;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) app += __shfl_xor(app, o);
        if (lane == 0) {
            atomicAdd((unsigned long long*)a.dbg + 0, (unsigned long long)d_slow);
            atomicAdd((unsigned long long*)a.dbg + 1, (unsigned long long)d_comp);
            atomicAdd((unsigned long long*)a.dbg + 2, (unsigned long long)app);
            atomicAdd((unsigned long long*)a.dbg + 3, (unsigned long long)ntiles);
            atomicAdd((unsigned long long*)a.dbg + 4, (unsigned long long)d_spill);      // spilled tiles (their cycles are part of clk_slow)
            atomicAdd((unsigned long long*)a.dbg + 5, d_clk_slow);
            atomicAdd((unsigned long long*)a.dbg + 6, d_clk_bar);
            atomicAdd((unsigned long long*)a.dbg + 8, d_clk_vm);
            if (w < 7) atomicAdd((unsigned long long*)a.dbg + 9 + w, d_clk_bar);     // barrier wait of waves 0..6 ("seg" + following words in the dump)
            atomicAdd((unsigned long long*)a.dbg + 7, (unsigned long long)(clock64() - d_clk_all));
            atomicAdd((unsigned long long*)a.dbg + 16, d_clk_pro);                   // pair prologue: barrier release -> step 0's fragment wait
        }
    }
    // ---- emit: best K' approximate candidates of this (chunk, query), sorted.  All 32 slots (DEEP: 8 at a time) are read back in ONE round trip (the query fragments are dead: registers are free).
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // spill launch: the list's fill count goes to memory once, here; a wave that never fell back has nothing in its slots and skips the emit
    if (spill_launch && lane == 0) a.spill_cnt[sp_list] = sp_cnt | (sp_live ? 0u : RMU_SPILL_FELL);
    const int part = s_idx;
    constexpr int GE = DEEP ? 8 : 32;
    // share_thr bit 2 (the ladder's FIRST launch: rmu_api.hip screen_enqueue): slots of at most K' entries are written as they are -- compact,
    // zeros behind them, NOT sorted -- and that launch's merge runs in its unsorted mode (topk_merge.hip).  A cold range is one tile per chunk,
    // every row a candidate: sorting 32 keys for each of a workgroup's 256 queries was ~25 us of VALU time in a launch that scans 2 000 rows.
    const bool emit_raw = (a.share_thr & 4) != 0;
    // (round 6, second session) ONE query tile (NWV = 4, batches <= 128 queries): the queries live in the first ceil(nq / 32) waves, and a slot
    // is sorted by a whole wave, one query after the other (rank_keys: n x ~8 instructions per query) -- a COLD range (the ladder's first: every
    // row of its tiles is a candidate, n = 32..40) kept ONE wave busy for ~1.6 us per query while three idled: 34 us of the batch-16 search and
    // 59 us of the batch-32 one (profiles/r06_search_timeline.txt).  The slots are in global memory, so any wave can sort any query: the
    // counts go through the waves' (now idle) threshold words in LDS and query q is emitted by wave q % 4.  Same keys, same ranks, same bytes.
    if constexpr (NWV == 4) {
        if (lane < 32) lds_store_b32(lds_addr(ssm + C::GT_OFF + w * 256) + (u32)lane * 4u, direct ? 0xffffffffu : cnt);   // (marker: the list is already written)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        const u32* call = (const u32*)(ssm + C::GT_OFF);
        for (int e0 = 0; e0 < 32; e0 += GE) {
            if (w + 4 * e0 >= a.nq) break;
            u64 key[GE][C::NPL];
            u32 nn[GE];
            bool done[GE];
#pragma unroll
            for (int e = 0; e < GE; ++e) {
                const int qq = w + 4 * (e0 + e);
                const bool ok = qq < a.nq;
                nn[e] = ok ? (u32)__builtin_amdgcn_readfirstlane((int)call[(qq >> 5) * 64 + (qq & 31)]) : 0u;
                done[e] = nn[e] == 0xffffffffu;
                if (done[e]) nn[e] = 0u;
                const u64* slot = a.gcand + ((size_t)s_idx * a.nq + (ok ? qq : 0)) * C::CAP;
#pragma unroll
                for (int pp = 0; pp < C::NPL; ++pp)
                    key[e][pp] = (u32)(lane + 64 * pp) < nn[e] ? __hip_atomic_load(slot + lane + 64 * pp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
            }
#pragma unroll
            for (int e = 0; e < GE; ++e) {
                const int qq = w + 4 * (e0 + e);
                if (qq < a.nq && !done[e]) {
                    u64* dst = a.partial + ((size_t)part * a.nq + qq) * a.k;
                    if (emit_raw && nn[e] <= (u32)a.k) {       // (uniform) the slot as it is, zeros behind it: the merge of this launch does not need it sorted
#pragma unroll
                        for (int pp = 0; pp < C::NPL; ++pp) {
                            const int le = lane + 64 * pp;
                            if (le < a.k) dst[le] = (u32)le < nn[e] ? key[e][pp] : 0ull;
                        }
                        continue;
                    }
                    u32 rank[C::NPL];
                    rank_keys<C::NPL>(key[e], nn[e], rank);
#pragma unroll
                    for (int pp = 0; pp < C::NPL; ++pp) {
                        const int le = lane + 64 * pp;
                        if ((u32)le < nn[e]) {
                            if (rank[pp] < (u32)a.k) dst[rank[pp]] = key[e][pp];
                        } else if (le < a.k) {
                            dst[le] = 0ull;
                        }
                    }
                }
            }
        }
    } else {
    for (int j0 = 0; j0 < 32; j0 += GE) {
        if (q_base + j0 >= a.nq || direct || (spill_launch && sp_live)) break;
        u64 key[GE][C::NPL];
        u32 nn[GE];
#pragma unroll
        for (int e = 0; e < GE; ++e) {
            const int jj = j0 + e;
            nn[e] = (u32)__builtin_amdgcn_readlane((int)cnt, qlane(jj));
            const u64* slot = (const u64*)(((u64)(u32)__builtin_amdgcn_readlane((int)(u32)((u64)gslot >> 32), qlane(jj)) << 32) |
                                           (u64)(u32)__builtin_amdgcn_readlane((int)(u32)(u64)gslot, qlane(jj)));
#pragma unroll
            for (int pp = 0; pp < C::NPL; ++pp)
                key[e][pp] = (u32)(lane + 64 * pp) < nn[e] ? __hip_atomic_load(slot + lane + 64 * pp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
        }
#pragma unroll
        for (int e = 0; e < GE; ++e) {
            const int qq = q_base + j0 + e;
            if (qq < a.nq) {
                u64* dst = a.partial + ((size_t)part * a.nq + qq) * a.k;
                if (emit_raw && nn[e] <= (u32)a.k) {
#pragma unroll
                    for (int pp = 0; pp < C::NPL; ++pp) {
                        const int le = lane + 64 * pp;
                        if (le < a.k) dst[le] = (u32)le < nn[e] ? key[e][pp] : 0ull;
                    }
                    continue;
                }
                u32 rank[C::NPL];
                rank_keys<C::NPL>(key[e], nn[e], rank);
#pragma unroll
                for (int pp = 0; pp < C::NPL; ++pp) {
                    const int le = lane + 64 * pp;
                    if ((u32)le < nn[e]) {
                        if (rank[pp] < (u32)a.k) dst[rank[pp]] = key[e][pp];
                    } else if (le < a.k) {
                        dst[le] = 0ull;
                    }
                }
            }
        }
    }
    }
}

// ---- K-SPLIT form of the screening scan, 128 queries per wave, round 3's kernel, the lean / lean2 steps: retired.  All bit-identical to
// the kernel above and none faster; their measurements are in NOTES_r01_r05.md 4.5 and profiles/r04_ab_screen_forms.txt.

// exact fp32 re-score of the K' candidates of each query, in the exact kernel's summation order:
// for t in 0..47, c in 0..3: acc = fma(x[8t+c], q[8t+c], acc); acc = fma(x[8t+4+c], q[8t+4+c], acc)
// (v_mfma_f32_32x32x2_f32 is a k-ordered fmaf chain; lanes < 32 hold k = 8t+c, lanes >= 32 hold k = 8t+4+c).
// L2 (RMU_METRIC_L2SQ; rows and queries `stride` = 768 floats apart, rows carry -|x|^2 in column 384, queries are (2q, 1): rmu_api.hip): the exact
// scan's chain runs on over the pad columns -- exact zeros except k = 384, the first term of step t = 48: S = fma(-|x|^2, 1, chain(2q, x)); the
// reported score is max(|q|^2 - S, 0) as in the exact path's merge (topk_merge.hip).  The candidates' approximate scores are HALF scores
// (q~.x~ - |x|^2 / 2: see scan_screen_lean3_kernel), the sufficiency test runs in those units: the image errors bound the q.x part as before,
// the norm is the SAME stored number on both sides, and the roundings that see it -- the screening chain starts at 2048 |x|^2 instead of 0
// (<= 408 roundings relative to |x||q| + |x|^2 / 2: 1.22e-5 |x|^2), the exact chain's last step rounds 2 q.x - |x|^2 once -- add 1.5e-5 |x|max^2.
template <bool L2, int NPL = 1>       // NPL: candidates per lane (K' <= 64 NPL); lane l holds candidates l, l + 64
__global__ __launch_bounds__(256) void k_rescore(const u64* __restrict__ cand, int kp, const float* __restrict__ x,
                                                 const float* __restrict__ q, int64_t nq, int k, float xnorm_max, float dx_max,
                                                 int64_t row_base, float* __restrict__ out_s, int64_t* __restrict__ out_r,
                                                 int* __restrict__ flagged /* [0] = number of queries that failed the test */,
                                                 int64_t* __restrict__ flagged_list /* their indices, in arrival order */,
                                                 float* __restrict__ eps_out /* optional [nq]: EPS(q) */, int stride,
                                                 const float* __restrict__ qn2_l2 /* L2: |q|^2 per query */) {
    const int lane = threadIdx.x & 63;
    const int64_t qi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= nq) return;
    u64 ck[NPL];
    bool valid[NPL];
    float sa[NPL], acc[NPL];
    u32 row[NPL];
    const float* xv[NPL];
#pragma unroll
    for (int p = 0; p < NPL; ++p) {
        ck[p] = lane + 64 * p < kp ? cand[qi * kp + lane + 64 * p] : 0ull;
        valid[p] = ck[p] != 0ull;
        sa[p] = valid[p] ? rmu_key_score(ck[p]) : -INFINITY;     // approximate score (sorted descending over the candidate index)
        row[p] = valid[p] ? rmu_key_row(ck[p]) : 0u;
        xv[p] = x + (int64_t)row[p] * stride;
        acc[p] = 0.f;
    }
    const float* qv = q + qi * stride;
    float qn2 = 0.f, dq2 = 0.f;
    // (round 6) the row pieces of UN steps are requested TOGETHER, then eaten in order: left as one load pair per step the 48-step chain of a
    // candidate paid a memory round trip per step (24-27 us per launch behind every search; the summation order is untouched)
    constexpr int UN = NPL == 1 ? 24 : 12;      // (second session: 12 / 6 -> 24 / 12 -- two round trips per candidate instead of four; 192 of the 256 registers a wave may take)
    for (int t0 = 0; t0 < SD / 8; t0 += UN) {
        f32x4 xa[NPL][UN], xb[NPL][UN];
#pragma unroll
        for (int u = 0; u < UN; ++u)
#pragma unroll
            for (int p = 0; p < NPL; ++p) {
                xa[p][u] = *(const f32x4*)(xv[p] + 8 * (t0 + u));
                xb[p][u] = *(const f32x4*)(xv[p] + 8 * (t0 + u) + 4);
            }
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int t = t0 + u;
            const f32x4 qa = *(const f32x4*)(qv + 8 * t), qb = *(const f32x4*)(qv + 8 * t + 4);
#pragma unroll
            for (int p = 0; p < NPL; ++p) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    acc[p] = fmaf(xa[p][u][c], qa[c], acc[p]);
                    acc[p] = fmaf(xb[p][u][c], qb[c], acc[p]);
                }
            }
            screen_eps_step<L2>(qa, qb, qn2, dq2);
        }
    }
    if (L2) {
#pragma unroll
        for (int p = 0; p < NPL; ++p) acc[p] = fmaf(xv[p][SD], qv[SD], acc[p]);
    }
    // sufficiency test on the approximate scores
    int nvalid = 0;
#pragma unroll
    for (int p = 0; p < NPL; ++p) nvalid += __builtin_popcountll(__ballot(valid[p]));
    auto approx_at = [&](int idx) -> float {                    // approximate score of candidate `idx` (uniform)
        float v = __shfl(sa[0], idx & 63);
#pragma unroll
        for (int p = 1; p < NPL; ++p) { const float vp = __shfl(sa[p], idx & 63); v = (idx >> 6) == p ? vp : v; }
        return v;
    };
    const float tau = approx_at(k - 1);                         // k-th best approximate score (or -inf)
    const float smin = approx_at(kp - 1);                       // worst kept candidate
    const float eps = screen_eps<L2>(qn2, dq2, xnorm_max, dx_max);
    const bool complete = nvalid < kp;                           // every live row was a candidate
    // eps must be finite: a query with |q_i| >= ~1000 overflows fp16(64 q), its approximate scores are inf/NaN and rows
    // scoring NaN are never appended (so even `complete` proves nothing) -- such a query always goes to the exact scan
    const bool ok = __builtin_isfinite(eps) && (complete || (smin < tau - 2.0f * eps));
    if (lane == 0) {
        if (!ok) flagged_list[atomicAdd(flagged, 1)] = qi;
        if (eps_out) eps_out[qi] = eps;
    }
    u64 key[NPL];
    u32 rank[NPL];
#pragma unroll
    for (int p = 0; p < NPL; ++p) key[p] = valid[p] ? rmu_make_key(acc[p] + 0.0f, row[p]) : 0ull;
    rank_keys<NPL>(key, (u32)(kp < 64 * NPL ? kp : 64 * NPL), rank);
    // keys of invalid lanes are 0 and rank below every valid one
#pragma unroll
    for (int p = 0; p < NPL; ++p) {
        if (valid[p] && rank[p] < (u32)k) {
            out_s[qi * k + rank[p]] = L2 ? fmaxf(qn2_l2[qi] - (acc[p] + 0.0f), 0.f) : acc[p] + 0.0f;
            out_r[qi * k + rank[p]] = (int64_t)row[p] + row_base;
        }
        const int le = lane + 64 * p;
        if (le < k && le >= nvalid) {
            out_s[qi * k + le] = L2 ? INFINITY : -INFINITY;
            out_r[qi * k + le] = -1;
        }
    }
}

}  // namespace

int rmu_split_launch(const float* src, void* dst, int64_t n_rows, hipStream_t s, int stride, float scale, u32* zero_a, int n_zero_a, u32* zero_b,
                     int n_zero_b, float* eps_out, float xnorm_max, float dx_max, int l2) {
    const int64_t groups = n_rows * (SD / 8);
    if (groups <= 0) return (n_zero_a > 0 || n_zero_b > 0 || eps_out) ? RMU_E_INVALID : RMU_OK;      // (the zeroing rides on a launch that exists)
    if (stride < SD) return RMU_E_INVALID;
    const int64_t conv_blocks = (groups + 255) / 256, eps_blocks = eps_out ? (n_rows + 255) / 256 : 0;
    if (eps_out && conv_blocks + eps_blocks > 0x7fffffff) return RMU_E_INVALID;
    hipLaunchKernelGGL(k_split_rows, dim3((unsigned)(conv_blocks + eps_blocks)), dim3(256), 0, s, src, (char*)dst, groups, stride, scale, zero_a,
                       zero_a ? n_zero_a : 0, zero_b, zero_b ? n_zero_b : 0, (int)(eps_out ? conv_blocks : 0x7fffffff), eps_out, n_rows, xnorm_max, dx_max,
                       l2);
    return hipGetLastError() == hipSuccess ? RMU_OK : RMU_E_HIP;
}

// geometry of one screening launch: scan_screen_lean3_kernel with 8 waves x 32 queries (full 256-query tiles) for batches over 128 queries,
// else 4 waves and ONE query tile; S row chunks (a multiple of 8 for the XCD-aware block map) so that grid = S * nqt fills the 256 CUs evenly
int rmu_screen_plan(ScanLaunch* p) {
    if (p->k < 1 || p->k > RMU_KS_CAP_DEEP - 8 || p->nq < 1 || p->n_rows < 0 || p->dpad != SD) return RMU_E_INVALID;   // (p->k is K': 32, 40, or up to 120 for 32 < k <= 104)
    // (The round-3 and round-4 forms of this kernel -- 4-wave G = 1/2, lean, lean2, K-split, 128 queries per wave -- were all bit-identical
    // and none faster; they were retired in favour of this one.  Their numbers: NOTES_r01_r05.md 4.5, profiles/r04_ab_screen_forms.txt.)
    p->wq = p->nq > 128 ? 8 : 4;
    p->qg = 1;
    p->kv = 4;
    const int qwg = 32 * p->wq;
    p->nqt = (p->nq + qwg - 1) / qwg;
    rmu_plan_chunks(p->nqt, (p->n_rows + S_RT - 1) / S_RT, &p->s_chunks, &p->tiles_per_chunk);
    p->grid = p->s_chunks * p->nqt;
    p->parts = p->s_chunks;
    static const int nt_env = rmu_env("RMU_NT") ? atoi(rmu_env("RMU_NT")) : 1;
    p->nt = (nt_env && p->nqt == 1) ? 1 : 0;            // one query tile: each image byte is read by one workgroup
    p->lds_bytes = p->wq == 8 ? Lean3Cfg<8>::LDS_BYTES : Lean3Cfg<4>::LDS_BYTES;   // (the DEEP forms take the same LDS)
    // sibling pacing (see the kernel): query tiles of a chunk on one XCD, 2..4 of them, the whole grid resident at once (these
    // kernels take > 80 KiB of LDS: one workgroup per CU), and enough tiles per workgroup for drift to matter
    // window in tiles (0 = off).  Measured (tools/pace_probe.py, 10M x 1024): 0 / 4 / 8 / 16 / 32 all 7.82-7.86 ms of scan kernels -- the pacing
    // costs nothing -- and on the round-4 boxes the siblings did not drift without it either (FETCH_SIZE 7.75-7.80 GB per batch = 1.01x
    // the image, L2 hit 0.758 with pacing off AND on; round 3's boxes: 15.1 GB, 0.53): kept on as the bound on that drift.
    static const int pace_env = rmu_env("RMU_SCREEN_PACE") ? atoi(rmu_env("RMU_SCREEN_PACE")) : 8;
    static const int n_cu = [] {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) n = 0;
        return n;
    }();
    p->pace = (pace_env > 0 && p->nqt >= 2 && p->nqt <= 4 && (p->s_chunks & 7) == 0 && p->grid <= n_cu &&
               p->tiles_per_chunk >= 4 * pace_env) ? pace_env : 0;
    return RMU_OK;
}

template <int EXP, int NWV, int NT, int L2N, bool DEEP = false>
static int screen_launch_lean3(const ScanLaunch* p, hipStream_t s) {
    return launch_cfg<Lean3Cfg<NWV, DEEP>, scan_screen_lean3_kernel<EXP, NWV, NT, L2N, DEEP>, 64 * NWV>(p, s);
}

int rmu_screen_launch(const ScanLaunch* p, hipStream_t s) {
    if (p->kv != 4 || !p->gcand) return RMU_E_INVALID;   // rmu_screen_plan hands out kv == 4 only
    const bool l2 = p->nrm != nullptr;                    // RMU_METRIC_L2SQ: the row norms enter the chain as its C operand
    if (p->k > RMU_KS_CAP - 8) {                          // deep K' (32 < k <= 104): slots of RMU_KS_CAP_DEEP keys
        if (p->wq == 4) {
            if (p->nt) return l2 ? screen_launch_lean3<0, 4, 1, 1, true>(p, s) : screen_launch_lean3<0, 4, 1, 0, true>(p, s);
            return l2 ? screen_launch_lean3<0, 4, 0, 1, true>(p, s) : screen_launch_lean3<0, 4, 0, 0, true>(p, s);
        }
        return l2 ? screen_launch_lean3<0, 8, 0, 1, true>(p, s) : screen_launch_lean3<0, 8, 0, 0, true>(p, s);
    }
    if (p->wq == 4) {                                     // one query tile
        if (p->nt) return l2 ? screen_launch_lean3<0, 4, 1, 1>(p, s) : screen_launch_lean3<0, 4, 1, 0>(p, s);
        return l2 ? screen_launch_lean3<0, 4, 0, 1>(p, s) : screen_launch_lean3<0, 4, 0, 0>(p, s);
    }
#ifdef RMU_DEBUG_KERNELS
    if (p->dbg && !l2) return screen_launch_lean3<4, 8, 0, 0>(p, s);   // cycle / event counters (RMU_SCAN_EXP=7: tools/screen_dbg_counters.py)
#endif
    return l2 ? screen_launch_lean3<0, 8, 0, 1>(p, s) : screen_launch_lean3<0, 8, 0, 0>(p, s);
}

int rmu_img_err_launch(const float* x, int64_t n_rows, float* err2, hipStream_t s, int stride) {
    if (n_rows <= 0) return RMU_OK;
    if (stride < SD) return RMU_E_INVALID;
    hipLaunchKernelGGL(k_img_err, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, s, x, n_rows, err2, stride);
    return hipGetLastError() == hipSuccess ? RMU_OK : RMU_E_HIP;
}

int rmu_rescore_launch(const u64* cand, int kp, const float* x, const float* q, int64_t nq, int k, float xnorm_max, float dx_max,
                       int64_t row_base, float* out_s, int64_t* out_r, int* flagged, int64_t* flagged_list, float* eps_out, hipStream_t s,
                       int stride, const float* qn2_l2) {
    if (kp < k || kp > 128 || stride < SD || (qn2_l2 && stride < SD + 1)) return RMU_E_INVALID;
    const dim3 grid((unsigned)((nq + 3) / 4));
    if (kp > 64) {       // deep K' (32 < k <= 104): two candidates per lane
        if (qn2_l2)
            hipLaunchKernelGGL((k_rescore<true, 2>), grid, dim3(256), 0, s, cand, kp, x, q, nq, k, xnorm_max, dx_max, row_base, out_s, out_r, flagged,
                               flagged_list, eps_out, stride, qn2_l2);
        else
            hipLaunchKernelGGL((k_rescore<false, 2>), grid, dim3(256), 0, s, cand, kp, x, q, nq, k, xnorm_max, dx_max, row_base, out_s, out_r, flagged,
                               flagged_list, eps_out, stride, qn2_l2);
    } else if (qn2_l2)
        hipLaunchKernelGGL((k_rescore<true, 1>), grid, dim3(256), 0, s, cand, kp, x, q, nq, k, xnorm_max, dx_max, row_base,
                           out_s, out_r, flagged, flagged_list, eps_out, stride, qn2_l2);
    else
        hipLaunchKernelGGL((k_rescore<false, 1>), grid, dim3(256), 0, s, cand, kp, x, q, nq, k, xnorm_max, dx_max, row_base,
                           out_s, out_r, flagged, flagged_list, eps_out, stride, qn2_l2);
    return hipGetLastError() == hipSuccess ? RMU_OK : RMU_E_HIP;
}

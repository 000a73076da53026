// scan_distinct.hip -- exact fp32 GROUPED top-k: the best row of each of the k best groups (gfx950 / MI355X only).
//
// Replaces: the grouping search the reference's stores offer and its callers build by hand -- Milvus col.search(group_by_field="source"),
//   LangChain's "parent document" retrieval in front of server/RAGHelper.py:497-499 -- so that one long document cannot fill every slot
//   of the retriever's k with its own chunks.
//
// One int32 code per row (a column of rmu_columns_t's device image) names the row's group.  The answer of a query: walk all live rows in
// rmu_index_search's order (score descending, then lower row id), keep a row iff no kept row has its code, stop at k.  Every score has
// the bits rmu_index_search gives the same row because scan_distinct_kernel is built from the SAME pieces of scan_common.h as
// scan_topk.hip and scan_subset.hip: the geometry (ScanGeom) and the swizzle of the LDS image, the block map, the A-fragment reads
// (afrag_base, afrag_read), the per-(wave, query) candidate slots in LDS (carve_slots, append_key, full_slots) and the final emit
// (emit_slots).  The query fragments sit in registers and the MFMA chain below issues v_mfma_f32_32x32x2_f32 in the k order documented
// at the head of scan_topk.hip.  What is this file's own:
//   * the tile loop: scan_subset.hip's without the gather -- contiguous rows, a scalar base per chunk as in scan_topk.hip, the filter of
//     a tile behind its own MFMA chain (no second accumulator);
//   * DISTINCT COMPACTION (compact_slots_distinct, beside scan_common.h's compact_slot): each lane fetches the code of its key's row,
//     a key is DOMINATED when a larger key of the slot has the same code, the survivors are ranked among themselves, the best k go back
//     sorted.  The slot's threshold becomes the k-th survivor's score ONLY when k survivors exist: until k distinct groups are known no
//     row may be pruned (a lower row can open a new group).  Dropping a dominated row is always safe -- a worse row of a group already
//     present is never in the answer -- and the strict `acc > thr` filter stays correct: a later row that ties the k-th group's score has
//     a higher id than everything this workgroup kept;
//   * the code lookup is an ordinary global load issued while LDS-DMA is in flight, so hipcc waits vmcnt(0) there and drains the ring.
//     That happens only inside a compaction; the counted waits of the tile loop stay valid afterwards (they only bound what may still be
//     outstanding);
//   * before the emit every slot of the wave is distinct-compacted once more, so every part list is sorted, internally distinct and at
//     most k long; emit_slots is used as it is;
//   * the shared thresholds (gthr) are neither published nor read: a bound would have to be a k-th DISTINCT best;
//   * k_distinct_fold turns the part lists [parts, nq, k] into one distinct list per query.  The union of the part lists contains the
//     answer: a group's global representative is the best row of its group in some part and is missing from that part's list only if k
//     better groups exist there.  A wave's running list (keys and codes) sits in lanes 0..31, the next part in lanes 32..63, the same
//     dominated / rank-the-survivors step runs over the 64 keys.  The first keys of 64 parts are fetched at once and a part whose first
//     key is below the running k-th (once k are held) is skipped with one compare, without touching its list.  One workgroup per query,
//     up to 16 waves (about 64 parts each), whose lists wave 0 folds at the end: one level, measured (profiles/distinct_search.md).
// Two geometries, k <= 32 only (CAP 64, one check per tile): WQ = 1 -- at most 32 queries, 128-row tiles, the four waves on different
// 32-row slices; WQ = 4 -- everything else, every wave on the same 32-row tile.
// Cost model: a workgroup whose row range holds fewer than k groups never gets a threshold -- every row of it is appended and every
// tile ends in compactions.  Correct, slow; DESIGN.md 4.1c.
#include "rmu_common.h"
#include "scan_common.h"
#include "../../include/rmu.h"

namespace {

// RING = 3: two chunks in flight; CAP 64, one check per tile
template <int D_, int WQ_, int CKF_>
struct DCfg : ScanGeom<D_, WQ_, CKF_, 3, 64, 1> {
    using G = ScanGeom<D_, WQ_, CKF_, 3, 64, 1>;
    static constexpr int LDS_BYTES = G::TAIL_OFF;
    static_assert(G::NCH >= 2, "the chunk requested in a step is at most one tile ahead");
    static_assert(G::NPL == 1, "compact_slots_distinct holds one key per lane and slot");
    static_assert(LDS_BYTES <= 160 * 1024, "LDS");
    static_assert(2 * G::NI <= 63, "vmcnt field");
};

extern __shared__ __attribute__((aligned(16))) char smem[];

__device__ __forceinline__ u64 readlane_u64(u64 v, int i) {
    return ((u64)(u32)__builtin_amdgcn_readlane((int)(u32)(v >> 32), i) << 32) | (u64)(u32)__builtin_amdgcn_readlane((int)(u32)v, i);
}

// One key per lane (0 = none; real keys are distinct) and the code of its row.  A key is DOMINATED when a larger key of the wave carries
// the same code.  *surv = the lanes whose key is real and not dominated; returns the number of SURVIVORS larger than this lane's key.
// Enumeration as rank_keys: key and code are broadcast with v_readlane, every lane compares.  Wave-uniform control flow only.
__device__ __forceinline__ u32 distinct_rank(u64 key, int code, u64& surv) {
    const u64 live = __ballot(key != 0ull);
    bool dom = false;
    for (u64 m = live; m;) {
        const int i = __builtin_ctzll(m);
        m &= m - 1;
        const u64 ki = readlane_u64(key, i);
        const int ci = __builtin_amdgcn_readlane(code, i);
        dom = dom || (ki > key && ci == code);
    }
    surv = __ballot(key != 0ull && !dom);
    u32 rank = 0;
    for (u64 m = surv; m;) {
        const int i = __builtin_ctzll(m);
        m &= m - 1;
        rank += readlane_u64(key, i) > key ? 1u : 0u;
    }
    return rank;
}

// compact_slot's distinct form: keep the best row of each of the best k groups of a slot (sorted, best first), refresh its count, and
// its threshold once k groups are held.  The slots named by `mask` (bit jj = slot jj) are taken DBATCH at a time: the code lookups of a
// batch are issued together, so their latency -- and the drain of the ring it stands for -- is paid once per batch, not once per slot
// (while no threshold exists, and at the emit, all 32 slots of a wave are due at once).  768-wide rows leave no registers for a batch
// (the query fragments alone are 384): one slot at a time there, anything more spills to scratch.
template <class C>
__device__ __forceinline__ void compact_slots_distinct(u32 mask, u64* cand_w, u32* cnt_w, float* thr_w, int k, int lane,
                                                       const int32_t* __restrict__ codes /* global: the group of every row */) {
    constexpr int DBATCH = C::D >= 768 ? 1 : 4;
    while (mask) {
        int jj[DBATCH];
        u64 key[DBATCH];
        int code[DBATCH];
#pragma unroll
        for (int b = 0; b < DBATCH; ++b) {
            jj[b] = mask ? __builtin_ctz(mask) : -1;
            mask &= mask - 1;                                  // (0 stays 0)
            key[b] = 0ull;
            if (jj[b] >= 0) {
                const u32 n_raw = cnt_w[jj[b]];
                const u32 n = n_raw < (u32)C::CAP ? n_raw : (u32)C::CAP;
                key[b] = ((u32)lane < n) ? cand_w[jj[b] * C::CAP + lane] : 0ull;
            }
        }
#pragma unroll
        for (int b = 0; b < DBATCH; ++b) code[b] = key[b] ? codes[rmu_key_row(key[b])] : -1;
#pragma unroll
        for (int b = 0; b < DBATCH; ++b) {
            if (jj[b] < 0) break;
            u64 surv;
            const u32 rank = distinct_rank(key[b], code[b], surv);
            const u32 ns = (u32)__popcll(surv);
            const u32 base = lds_addr(cand_w + jj[b] * C::CAP);
            if (((surv >> lane) & 1ull) && rank < (u32)k) {
                lds_store_b64(base + rank * 8u, key[b]);
                if (rank == (u32)(k - 1)) lds_store_b32(lds_addr(thr_w + jj[b]), __float_as_uint(rmu_key_score(key[b])));
            }
            if (lane == 0) lds_store_b32(lds_addr(cnt_w + jj[b]), ns < (u32)k ? ns : (u32)k);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
}

template <class C>
__global__ __launch_bounds__(256) void scan_distinct_kernel(const DistinctLaunch a) {
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = w % C::WQ;   // query group of this wave
    const int rp = w / C::WQ;  // row part of this wave
    const int h = lane >> 5;
    const int j = lane & 31;

    int s_idx, qt;   // corpus chunk, query tile
    block_map(a.s_chunks, a.nqt, s_idx, qt);
    const int64_t tiles_total = (a.n_rows + C::RT - 1) / C::RT;
    const int64_t t0 = (int64_t)s_idx * a.tiles_per_chunk;
    int64_t t1 = t0 + a.tiles_per_chunk;
    if (t1 > tiles_total) t1 = tiles_total;
    const int ntiles = (int)(t1 > t0 ? t1 - t0 : 0);

    char* ring = smem;
    const int q_base = (qt * C::WQ + g) * 32, q_idx = q_base + j;
    const bool q_ok = q_idx < a.nq;
    u64* cand_w;
    u32* cnt_w;
    float* thr_w;
    carve_slots<C>(smem, w, lane, q_ok, cand_w, cnt_w, thr_w);
    float thr = q_ok ? -INFINITY : INFINITY;

    // ---- query fragments -> registers, as scan_topk_kernel (padded query columns read row 0: their threshold is +inf).  One copy per
    // kernel: see the head of scan_common.h -------------------------------------------------------------------------------------------
    f32x4 qf[C::D / 8];
    {
        const float* qrow = a.q + (size_t)(q_ok ? q_idx : 0) * C::D + 4 * h;
#pragma unroll
        for (int t = 0; t < C::D / 8; ++t) qf[t] = *(const f32x4*)(qrow + 8 * t);
    }

    // ---- per-lane DMA source map, as scan_topk_kernel: byte offset of this lane's (de-swizzled) 16-B unit inside a [RT x D] tile; the
    // per-chunk base is a scalar.  Rows past n_rows are read (the index keeps >= 128 slack rows) and dropped by the filter.
    u32 dma_off[C::NI];
#pragma unroll
    for (int n = 0; n < C::NI; ++n) {
        const int f = (n * 4 + w) * 64 + lane;
        const int i = f / C::U16, p = f % C::U16;
        dma_off[n] = (u32)(i * C::D + 4 * (p ^ swz(i, C::SWB))) * 4u;
    }
    auto issue_chunk = [&](int tl, int c, int slot) {   // chunk c of tile tl of this workgroup -> ring slot
        if (tl >= ntiles) tl = ntiles - 1;              // tail: harmless reloads keep the vmcnt bookkeeping uniform
        const char* sbase = (const char*)(a.x + ((t0 + tl) * C::RT) * (int64_t)C::D + c * C::CKF);
        char* dst = ring + slot * C::SLOT_BYTES;
#pragma unroll
        for (int n = 0; n < C::NI; ++n)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(sbase + dma_off[n]),
                                             (__attribute__((address_space(3))) void*)(dst + (n * 4 + w) * 1024), 16, 0, 0);
    };

    const int rowi = 32 * rp + j;
    int abase[C::SWB / 2];
#pragma unroll
    for (int m = 0; m < C::SWB / 2; ++m) abase[m] = afrag_base<C>(rowi, h, m);
    auto read_frag = [&](int slot_off, int t) -> f32x4 { return afrag_read<C>(ring, abase, slot_off, t); };

    const u32 cnt_addr = lds_addr(cnt_w + j);
    const u32 cand_addr = lds_addr(cand_w + j * C::CAP);
    const u32 trash_addr = lds_addr(smem + C::TRASH_OFF) + threadIdx.x * 8u;

    auto check_compact = [&]() {
        const u32 mask = full_slots<C>(cnt_w, j);
        if (mask) {
            compact_slots_distinct<C>(mask, cand_w, cnt_w, thr_w, a.k, lane, a.codes);
            thr = thr_w[j];
        }
    };
    // append the rows of `acc` that pass (pmask) to this lane's query slot.  All LDS writes are inline asm: a compiler-generated LDS
    // write is ordered behind the in-flight LDS-DMA with s_waitcnt vmcnt(0) and would drain the ring (scan_topk.hip).
    auto append_round = [&](const f32x16& acc, u32 pmask, u32 row0) {
        const u32 n = __builtin_popcount(pmask);
        u32 res_pos;
        asm volatile("ds_add_rtn_u32 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=v"(res_pos) : "v"(cnt_addr), "v"(n) : "memory");
        u32 wr_addr = cand_addr + res_pos * 8u;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const u64 key = rmu_make_key(acc[r] + 0.0f, row0 + (u32)((r & 3) + 8 * (r >> 2)));
            const bool pass = (pmask >> r) & 1u;
            append_key(pass, wr_addr, trash_addr, key);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        check_compact();
    };

    if (ntiles > 0) {
        issue_chunk(0, 0, 0);
        issue_chunk(0, 1, 1);
        // the query fragments are taken HERE, behind the prologue's requests: hipcc otherwise places its own wait for them -- vmcnt(0),
        // it cannot count across the inline-asm waits below -- in front of the first MFMA of EVERY tile and drains the ring there
#pragma unroll
        for (int t = 0; t < C::D / 8; ++t) asm volatile("" ::"v"(qf[t]));
        int slot = 0, islot = 2;     // ring slot of the chunk computed / requested in this step
        for (int tl = 0; tl < ntiles; ++tl) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
            for (int c = 0; c < C::NCH; ++c) {
                // own DMA of this chunk (and of everything older) has landed; own LDS reads have returned
                asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(C::NI) : "memory");
                __builtin_amdgcn_s_barrier();
                issue_chunk(tl + (c + 2) / C::NCH, (c + 2) % C::NCH, islot);   // refills the slot every wave finished reading last step
                const int slot_off = slot * C::SLOT_BYTES;
                f32x4 a_cur = read_frag(slot_off, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
#pragma unroll
                for (int t = 0; t < C::TS; ++t) {
                    f32x4 a_nxt = a_cur;
                    if (t + 1 < C::TS) a_nxt = read_frag(slot_off, t + 1);
                    const f32x4 qv = qf[c * C::TS + t];
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur.x, qv.x, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur.y, qv.y, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur.z, qv.z, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur.w, qv.w, acc, 0, 0, 0);
                    a_cur = a_nxt;
                    // pin the software pipeline: the NEXT fragment's ds_read issues ahead of this step's four MFMAs (hipcc otherwise
                    // sinks it behind them and exposes the LDS round trip)
                    if (t + 1 < C::TS) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
                }
                slot = slot == C::RING - 1 ? 0 : slot + 1;
                islot = islot == C::RING - 1 ? 0 : islot + 1;
            }
            // ---- filter of this tile: tombstoned (NaN) rows never pass; rows past the last one exist only in the globally last tile
            u32 pmask = 0;
#pragma unroll
            for (int r = 0; r < 16; ++r) pmask |= (acc[r] > thr) ? (1u << r) : 0u;
            const int64_t row0 = (t0 + tl) * C::RT + 32 * rp + 4 * h;      // this lane's first row of the tile
            if ((t0 + tl + 1) * C::RT > a.n_rows) {
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (row0 + (r & 3) + 8 * (r >> 2) >= a.n_rows) pmask &= ~(1u << r);
            }
            if (__any(pmask != 0)) append_round(acc, pmask, (u32)row0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }

    // every slot of the wave distinct and at most k long, then the shared emit
    {
        const int nslots = a.nq - q_base < 32 ? a.nq - q_base : 32;
        if (C::D >= 768) {                                     // (slot by slot: the form hipcc keeps in registers at this width)
            for (int jj = 0; jj < nslots; ++jj) compact_slots_distinct<C>(1u << jj, cand_w, cnt_w, thr_w, a.k, lane, a.codes);
        } else if (nslots > 0) {
            compact_slots_distinct<C>(nslots >= 32 ? 0xFFFFFFFFu : (1u << nslots) - 1u, cand_w, cnt_w, thr_w, a.k, lane, a.codes);
        }
    }
    emit_slots<C>(cand_w, cnt_w, a.partial, s_idx * C::RP + rp, q_base, a.nq, a.nq, a.k, lane);
}

// One fold step: lanes 0..31 hold the running list (best first, zeros last), lanes 32..63 a part list; afterwards lanes 0..31 hold the best
// key of each of the k best groups of the 64, sorted, and lanes 32..63 nothing.  A survivor PUSHES its key and code to the lane of its
// rank (ds_permute: a lane nobody writes to receives 0, which is the padding); everything else goes to lane 63, which is cleared.
__device__ __forceinline__ void fold_step(u64& key, int& code, int k, int lane) {
    u64 surv;
    const u32 rank = distinct_rank(key, code, surv);
    const int dst = ((((surv >> lane) & 1ull) && rank < (u32)k) ? (int)rank : 63) * 4;
    const u32 lo = (u32)__builtin_amdgcn_ds_permute(dst, (int)(u32)key), hi = (u32)__builtin_amdgcn_ds_permute(dst, (int)(u32)(key >> 32));
    const int cd = __builtin_amdgcn_ds_permute(dst, code);
    key = lane < 32 ? (((u64)hi << 32) | lo) : 0ull;
    code = lane < 32 ? cd : -1;
}

// part lists [parts, nq, k] (each sorted, distinct inside, zeros last) -> out [nq, k]: the best key of each of the k best groups of
// their union, sorted, zero-padded.  One workgroup of W = blockDim.x / 64 waves per query (see the head of this file): wave w folds parts
// w, w + W, ... -- the first keys of 64 of them fetched at once --, parks its list in LDS, and wave 0 folds the W lists.
__global__ __launch_bounds__(1024) void k_distinct_fold(const u64* __restrict__ partial, int parts, int nq, int k, const int32_t* __restrict__ codes,
                                                        u64* __restrict__ out) {
    __shared__ u64 s_key[16][32];
    __shared__ int s_code[16][32];
    const int q = blockIdx.x, lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), W = blockDim.x >> 6;
    u64 key = 0ull;     // lanes 0..31: the running list, best first; lanes 32..63: the part being folded
    int code = -1;
    u64 kth = 0ull;     // the running k-th key once k groups are held (0: fewer)
    const int mine = parts > w ? (parts - w + W - 1) / W : 0;       // parts of this wave: w + i W
    for (int i0 = 0; i0 < mine; i0 += 64) {
        const int lim = mine - i0 < 64 ? mine - i0 : 64;
        const u64 first = lane < lim ? partial[((size_t)(w + (i0 + lane) * W) * nq + q) * k] : 0ull;
        for (int i = 0; i < lim; ++i) {
            const u64 f = readlane_u64(first, i);
            if (f == 0ull || f < kth) continue;      // an empty part, or a sorted list none of which can enter
            if (lane >= 32) {
                const int e = lane - 32;
                key = e < k ? partial[((size_t)(w + (i0 + i) * W) * nq + q) * k + e] : 0ull;
                code = key ? codes[rmu_key_row(key)] : -1;
            }
            fold_step(key, code, k, lane);
            kth = readlane_u64(key, k - 1);
        }
    }
    if (lane < 32) { s_key[w][lane] = key; s_code[w][lane] = code; }
    __syncthreads();
    if (w != 0) return;
    for (int v = 1; v < W; ++v) {
        if (lane >= 32) { key = s_key[v][lane - 32]; code = s_code[v][lane - 32]; }
        fold_step(key, code, k, lane);
    }
    if (lane < k) out[(size_t)q * k + lane] = key;
}

// geometry table: k <= 32 only.       D   WQ  CKF
template <int D> using D_w1 = DCfg<D, 1, 48>;                    // 72 KiB ring (48 KiB in flight) + 64 KiB candidates
template <int D> using D_w4 = DCfg<D, 4, D == 192 ? 32 : 96>;    // 36 KiB ring (192-wide rows: 12 KiB, six chunks per tile)

template <int D, class F>
int with_cfg(int wq, F&& f) {
    switch (wq) {
        case 1: return f(D_w1<D>{});
        case 4: return f(D_w4<D>{});
        default: return RMU_E_INVALID;
    }
}

}  // namespace

int rmu_distinct_plan(DistinctLaunch* p) {
    if (p->k < 1 || p->k > RMU_MAX_K_DISTINCT || p->nq < 1 || p->n_rows < 1 || p->n_rows >= 0xFFFFFFFFll) return RMU_E_INVALID;
    if (p->dpad != 192 && p->dpad != 384 && p->dpad != 768) return RMU_E_INVALID;
    p->wq = p->nq <= 32 ? 1 : 4;
    const int rt = 32 * (4 / p->wq);
    p->nqt = (p->nq + 32 * p->wq - 1) / (32 * p->wq);
    // corpus chunks as rmu_scan_plan's
    rmu_plan_chunks(p->nqt, (p->n_rows + rt - 1) / rt, &p->s_chunks, &p->tiles_per_chunk);
    p->grid = p->s_chunks * p->nqt;
    p->parts = p->s_chunks * (4 / p->wq);
    p->lds_bytes = for_dpad(p->dpad, [&](auto d) { return with_cfg<decltype(d)::value>(p->wq, [](auto c) { return (int)decltype(c)::LDS_BYTES; }); });
    return p->lds_bytes > 0 ? RMU_OK : RMU_E_INVALID;
}

int rmu_distinct_launch(const DistinctLaunch* p, hipStream_t s) {
    return for_dpad(p->dpad, [&](auto d) {
        return with_cfg<decltype(d)::value>(p->wq, [&](auto c) { return launch_cfg<decltype(c), scan_distinct_kernel<decltype(c)>>(p, s); });
    });
}

int rmu_distinct_fold_launch(const u64* partial, int parts, int64_t nq, int k, const int32_t* codes, u64* out_keys, hipStream_t s) {
    if (parts < 1 || parts > 1024 || nq < 1 || k < 1 || k > RMU_MAX_K_DISTINCT) return RMU_E_INVALID;
    // waves per query: about 64 parts each (one fetch of first keys), at most 16; many queries fill the device by themselves
    int waves = (parts + 63) / 64;
    if (nq >= 2048 && waves > 4) waves = 4;
    hipLaunchKernelGGL(k_distinct_fold, dim3((unsigned)nq), dim3(64 * waves), 0, s, partial, parts, (int)nq, k, codes, out_keys);
    return hipGetLastError() == hipSuccess ? RMU_OK : RMU_E_HIP;
}

// scan_wide.hip -- exact fp32 fused scan + top-k for rows wider than the register-resident scans hold (gfx950 / MI355X only).
//
// Serves: the same FLAT similarity search as scan_topk.hip (server/RAGHelper.py:497-499) for the `embedding_model`s the reference
// accepts beyond 768 dimensions (server/RAGHelper_local.py:107-117, .env.template:3): bge-large / e5-large / bge-m3 (1024-d),
// OpenAI-style 1536-d and 3072-d vectors.
//
// scan_topk_kernel keeps the fragments of a wave's 32 queries in registers (D/2 VGPRs): 768 floats are 384 of the wave's 512.  Here
// the queries are STREAMED: a ring slot is a K-chunk of the tile's rows plus the same K-chunk of the workgroup's queries, both filled
// by LDS-DMA (global_load_lds, 16-byte units, source address swizzled per lane, counted vmcnt), and both MFMA operands are ds_read
// from it.  The row width is a run-time loop count (dpad / CKF chunks per tile): one set of instantiations serves every width.
//
// What is the exact scan's, unchanged: v_mfma_f32_32x32x2_f32 with lane l owning query (l & 31); the k-permutation (lane (i, h) multiplies
// component c of the float4 at 8t + 4h, t ascending over the whole row, ONE accumulator chain per (row, query): a score has the bits
// scan_topk_kernel gives it, whatever the batch, k, geometry or row range); keys rmu_make_key(score + 0.0f, row); the candidate slots in
// LDS and their append / compact / emit protocol (scan_common.h); the shared thresholds, the device predicate, row0; ScanLaunch.
//
// What is simpler: the threshold filter of a tile runs at the tile's end, not inside the next tile's MFMA gaps.  A tile is dpad / 2
// MFMAs of 64 cycles (>= 24 576 cycles at 768, 98 304 at 3072); draining the pipe and 16 compares once per tile is < 1% of that, and
// the two alternating accumulators, the per-gap mask bits and the peeled loop of scan_topk_kernel have nothing left to hide.
//
// Tile shapes: those of the exact scan -- WQ = 4: 32 rows x 128 queries per workgroup, WQ = 2: 64 x 64, WQ = 1: 128 x 32
// (row parts spread over the four waves, non-temporal row stream when there is one query tile).  k > 32 (120-deep candidate slots,
// 120 KiB) leaves room for three 8-KiB slots only: 64 x 64 tiles in 16-float chunks, whatever the batch.
#include "rmu_common.h"
#include "scan_common.h"
#include "../../include/rmu.h"

namespace {

// LDS: [ring of (row chunk | query chunk) slots][candidate slots][counts][thresholds][trash][landing zone of the shared thresholds]
template <int WQ_, int CKF_, int RING_, int CAP_, int NCHECK_, int NT_>
struct WCfg {
    static constexpr int WQ = WQ_;              // query groups per workgroup
    static constexpr int RP = 4 / WQ_;          // row parts per tile
    static constexpr int RT = 32 * RP;          // rows per tile
    static constexpr int NQ = 32 * WQ_;         // queries per workgroup
    static constexpr int CKF = CKF_;            // floats per K-chunk
    static constexpr int U16 = CKF_ / 4;        // 16-byte units per row (or query) of a chunk
    static constexpr int TS = CKF_ / 8;         // K-steps (one ds_read_b128 per operand, four MFMAs) per chunk
    static constexpr int RING = RING_;
    static constexpr int ROWS_BYTES = RT * CKF_ * 4;             // the row chunk's image; the query chunk's follows it
    static constexpr int SLOT_BYTES = (RT + NQ) * CKF_ * 4;
    static constexpr int NI_ROWS = RT * U16 / 256;               // DMA wave-instructions per wave per chunk: rows ...
    static constexpr int NI = (RT + NQ) * U16 / 256;             // ... and in all
    static constexpr int CAP = CAP_;
    static constexpr int NPL = (CAP_ + 63) / 64;
    static constexpr int NCHECK = NCHECK_;
    static constexpr int A = 32 / NCHECK_;      // max appends per slot between overflow checks
    static constexpr int SWB = (U16 % 16 == 8) ? 8 : 4;          // swizzle block (units)
    static constexpr bool NT = NT_ != 0;        // rows are read by exactly one workgroup: non-temporal stream
    static constexpr int RING_BYTES = RING_ * SLOT_BYTES;
    static constexpr int CAND_BYTES = 4 * 32 * CAP_ * 8;
    static constexpr int CNT_OFF = RING_BYTES + CAND_BYTES;
    static constexpr int THR_OFF = CNT_OFF + 4 * 32 * 4;
    static constexpr int TRASH_OFF = THR_OFF + 4 * 32 * 4;       // one private 8-B trash slot per lane
    static constexpr int GT_OFF = TRASH_OFF + 256 * 8;           // per-wave landing zone of the shared thresholds
    static constexpr int LDS_BYTES = GT_OFF + 4 * 256;
    static constexpr int WAITN = NI * (RING_ - 2);               // DMA instructions that may stay in flight across a chunk's barrier
    static_assert(LDS_BYTES <= 160 * 1024, "LDS");
    static_assert(CKF_ % 8 == 0 && (RT * U16) % 256 == 0 && (NQ * U16) % 256 == 0, "DMA split: whole wave-instructions of rows, then of queries");
    static_assert(U16 % 16 == 8 || U16 % 16 == 4, "swizzle classes");
    // RING <= 3: the 4-byte refresh of the shared thresholds is issued in front of a tile's last chunk group and must lie outside the
    // RING - 2 groups the counted wait leaves in flight one chunk later
    static_assert(RING_ >= 2 && RING_ <= 3 && WAITN <= 63, "vmcnt bookkeeping");
};

extern __shared__ __attribute__((aligned(16))) char smem[];

template <class C>
__global__ __launch_bounds__(256) void scan_wide_kernel(const ScanLaunch a) {
    // device-side launch predicate, as scan_topk_kernel's: uniform over the grid
    int nq_eff = a.nq;
    if (a.cond.p) {
        const int c = *a.cond.p;
        if (c < a.cond.lo || c > a.cond.hi) return;
        if (a.cond.clamp && c < nq_eff) nq_eff = c;
    }
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = w % C::WQ;   // query group of this wave
    const int rp = w / C::WQ;  // row part of this wave
    const int h = lane >> 5;
    const int j = lane & 31;
    const int dpad = a.dpad;
    const int nch = dpad / C::CKF;   // chunks per tile

    int s_idx, qt;   // corpus chunk, query tile
    block_map(a.s_chunks, a.nqt, s_idx, qt);
    const int64_t tiles_total = (a.n_rows + C::RT - 1) / C::RT;
    const int64_t t0 = (int64_t)s_idx * a.tiles_per_chunk;
    int64_t t1 = t0 + a.tiles_per_chunk;
    if (t1 > tiles_total) t1 = tiles_total;
    const int ntiles = (int)(t1 > t0 ? t1 - t0 : 0);

    char* ring = smem;
    const int q_base = (qt * C::WQ + g) * 32, q_idx = q_base + j;
    const bool q_ok = q_idx < nq_eff;
    ((u32*)(smem + C::GT_OFF))[w * 64 + lane] = 0u;   // landing zone of the shared thresholds: 0 = no bound
    u64* cand_w;
    u32* cnt_w;
    float* thr_w;
    carve_slots<C>(smem, w, lane, q_ok, cand_w, cnt_w, thr_w);
    float thr = q_ok ? -INFINITY : INFINITY;       // effective filter = max(local k-th best, shared bound)
    float thr_loc = thr, thr_g = -INFINITY;
    u32* gthr_w = a.gthr + q_base;
    const u32* gt_lds = (const u32*)(smem + C::GT_OFF) + w * 64;

    // ---- per-lane DMA source map (constant over the kernel): byte offset of this lane's 16-B unit, de-swizzled, inside the tile's
    // [RT x dpad] rows (instructions n < NI_ROWS) or inside the query matrix (the others).  Rows past n_rows are read (the index keeps
    // >= 128 slack rows) and blanked by the filter; query columns past nq_eff read query 0: their threshold is +inf, nothing is emitted.
    u32 dma_off[C::NI];
#pragma unroll
    for (int n = 0; n < C::NI; ++n) {
        const int f = ((n < C::NI_ROWS ? n : n - C::NI_ROWS) * 4 + w) * 64 + lane;
        const int i = f / C::U16, p = f % C::U16;
        if (n < C::NI_ROWS) {
            dma_off[n] = ((u32)i * (u32)dpad + 4u * (u32)(p ^ swz(i, C::SWB))) * 4u;
        } else {
            const int qg = qt * C::NQ + i;
            dma_off[n] = ((u32)(qg < nq_eff ? qg : 0) * (u32)dpad + 4u * (u32)(p ^ swz(i, C::SWB))) * 4u;
        }
    }
    // running position of the DMA stream: tile, chunk inside it, ring slot
    int i_tl = 0, i_c = 0, i_slot = 0;
    auto issue_chunk = [&]() {
        const int tl = i_tl < ntiles ? i_tl : ntiles - 1;   // tail: harmless reloads keep the vmcnt bookkeeping uniform
        const char* xb = (const char*)(a.x + ((t0 + tl) * C::RT) * (int64_t)dpad + i_c * C::CKF);
        const char* qb = (const char*)(a.q + i_c * C::CKF);
        char* slot = ring + i_slot * C::SLOT_BYTES;
#pragma unroll
        for (int n = 0; n < C::NI; ++n) {
            // (the aux operand must be a literal)
            if (n < C::NI_ROWS && C::NT)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(xb + dma_off[n]),
                                                 (__attribute__((address_space(3))) void*)(slot + (n * 4 + w) * 1024), 16, 0, 2);
            else
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)((n < C::NI_ROWS ? xb : qb) + dma_off[n]),
                                                 (__attribute__((address_space(3))) void*)(slot + (n * 4 + w) * 1024), 16, 0, 0);
        }
        if (++i_c == nch) { i_c = 0; ++i_tl; }
        if (++i_slot == C::RING) i_slot = 0;
    };

    // fragment read offsets inside a slot: A = row (32 rp + j) of the row image, B = query (32 g + j) of the query image
    int abase[C::SWB / 2], bbase[C::SWB / 2];
#pragma unroll
    for (int m = 0; m < C::SWB / 2; ++m) {
        abase[m] = afrag_base<C>(32 * rp + j, h, m);
        bbase[m] = C::ROWS_BYTES + afrag_base<C>(32 * g + j, h, m);
    }

    const u32 cnt_addr = lds_addr(cnt_w + j);
    const u32 cand_addr = lds_addr(cand_w + j * C::CAP);
    const u32 trash_addr = lds_addr(smem + C::TRASH_OFF) + threadIdx.x * 8u;

    auto check_compact = [&]() {
        u32 mask = full_slots<C>(cnt_w, j);
        if (mask) {
            while (mask) {
                const int jj = __builtin_ctz(mask);
                mask &= mask - 1;
                compact_slot<C>(jj, cand_w, cnt_w, thr_w, a.k, lane, gthr_w);
            }
            thr_loc = thr_w[j];
            thr = fmaxf(thr_loc, thr_g);
        }
    };

    // ---- threshold filter of one finished tile.  Every LDS store is inline asm (scan_common.h): the ring is not drained. ----------
    auto filter_tile = [&](const f32x16& acc, int64_t rbase, bool last) {
        u32 pmask = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) pmask |= (acc[r] > thr) ? (1u << r) : 0u;     // tombstoned rows are NaN and never pass
        if (last) {   // rows >= n_rows exist only in a chunk's last tile
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (rbase + (r & 3) + 8 * (r >> 2) >= a.n_rows) pmask &= ~(1u << r);
        }
        if (!__any(pmask != 0)) return;
#pragma unroll
        for (int half = 0; half < C::NCHECK; ++half) {
            const int r0 = half * (16 / C::NCHECK), r1 = r0 + 16 / C::NCHECK;
            const u32 bits = ((1u << (r1 - r0)) - 1u) << r0;
            const u32 n = __builtin_popcount(pmask & bits);
            u32 res_pos;
            asm volatile("ds_add_rtn_u32 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=&v"(res_pos) : "v"(cnt_addr), "v"(n) : "memory");
            u32 wr_addr = cand_addr + res_pos * 8u;
#pragma unroll
            for (int r = r0; r < r1; ++r) {
                const u64 key = rmu_make_key(acc[r] + 0.0f, (u32)(a.row0 + rbase + (r & 3) + 8 * (r >> 2)));
                append_key((pmask >> r) & 1u, wr_addr, trash_addr, key);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            check_compact();
        }
    };

    if (ntiles > 0) {
        // ---- prologue: RING - 1 chunks in flight ----------------------------------------------------
#pragma unroll
        for (int c0 = 0; c0 < C::RING - 1; ++c0) issue_chunk();
        const int64_t lane_r0 = t0 * C::RT + 32 * rp + 4 * h;   // this lane's first row in tile 0
        int slot = 0;
        for (int tl = 0; tl < ntiles; ++tl) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            for (int c = 0; c < nch; ++c) {
                // own DMA of this chunk has landed; own LDS reads of the last one have returned
                asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(C::WAITN) : "memory");
                __builtin_amdgcn_s_barrier();
                if (c == 0) {
                    // shared threshold fetched by the last tile's DMA: pass iff v >= bound  <=>  v > nextbelow(bound)
                    const u32 go = gt_lds[j];
                    thr_g = (go && a.share_thr) ? rmu_ord2f(go - 1u) : -INFINITY;
                    thr = fmaxf(thr_loc, thr_g);
                }
                if (c == nch - 1) {
                    // refresh for the next tile: one 4-B-per-lane LDS-DMA, issued BEFORE this chunk's group so the next counted
                    // vmcnt covers it; sc1 = skip the (never refreshed) per-CU L1
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gthr_w + j),
                                                     (__attribute__((address_space(3))) void*)(smem + C::GT_OFF + w * 256), 4, 0, 16);
                }
                issue_chunk();   // refills the slot every wave finished reading before the barrier
                const int slot_off = slot * C::SLOT_BYTES;
                f32x4 av[C::TS], bv[C::TS];
#pragma unroll
                for (int t = 0; t < C::TS; ++t) {
                    av[t] = afrag_read<C>(ring, abase, slot_off, t);
                    bv[t] = afrag_read<C>(ring, bbase, slot_off, t);
                }
#pragma unroll
                for (int t = 0; t < C::TS; ++t) {
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t].x, bv[t].x, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t].y, bv[t].y, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t].z, bv[t].z, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t].w, bv[t].w, acc, 0, 0, 0);
                }
                if (++slot == C::RING) slot = 0;
            }
            filter_tile(acc, lane_r0 + (int64_t)tl * C::RT, tl == ntiles - 1);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }

    emit_slots<C>(cand_w, cnt_w, a.partial, s_idx * C::RP + rp, q_base, nq_eff, a.nq, a.k, lane);
}

// dispatch table: (query geometry) x (k class) x (non-temporal).  kv 0: k <= 32 (CAP 64, one check per tile); kv 1: k <= 112 (CAP 120, a check every four rows).
//                          WQ CKF RING CAP NCHECK NT
using W_w4_k0 = WCfg<4, 32, 3, 64, 1, 0>;      // 60 KiB ring + 64 KiB candidates
using W_w2_k0 = WCfg<2, 32, 3, 64, 1, 0>;      // 48 KiB ring
using W_w1_k0 = WCfg<1, 32, 3, 64, 1, 0>;      // 60 KiB ring
// one query tile (<= 64 queries): every corpus byte is read by exactly one workgroup -> non-temporal row stream
using W_w2_k0_nt = WCfg<2, 32, 3, 64, 1, 1>;
using W_w1_k0_nt = WCfg<1, 32, 3, 64, 1, 1>;
using W_w2_k1 = WCfg<2, 16, 3, 120, 4, 0>;     // 24 KiB ring + 120 KiB candidates: four checks per appending tile, 112 kept + 8 free

template <class F>
int with_wcfg(int wq, int kv, int nt, F&& f) {
    switch (wq * 2 + kv) {
        case 8: return f(W_w4_k0{});
        case 4: return nt ? f(W_w2_k0_nt{}) : f(W_w2_k0{});
        case 2: return nt ? f(W_w1_k0_nt{}) : f(W_w1_k0{});
        case 5: return f(W_w2_k1{});
        default: return RMU_E_INVALID;
    }
}

}  // namespace

// grid, parts and LDS bytes of one scan_wide_kernel launch (rmu_scan_plan routes here: dpad > 768, or ScanLaunch::wide set by the caller)
int rmu_wide_plan(ScanLaunch* p) {
    if (p->k < 1 || p->k > RMU_MAX_K || p->nq < 1 || p->n_rows < 0) return RMU_E_INVALID;
    if (p->dpad < 64 || p->dpad > RMU_MAX_DIM_WIDE || p->dpad % 32 != 0) return RMU_E_INVALID;
    p->wide = 1;
    p->kv = p->k <= 32 ? 0 : 1;
    p->wq = p->kv == 1 ? 2 : (p->nq <= 32 ? 1 : (p->nq <= 64 ? 2 : 4));
    const int rt = 32 * (4 / p->wq);
    p->nqt = (p->nq + 32 * p->wq - 1) / (32 * p->wq);
    rmu_plan_chunks(p->nqt, (p->n_rows + rt - 1) / rt, &p->s_chunks, &p->tiles_per_chunk);
    p->grid = p->s_chunks * p->nqt;
    p->parts = p->s_chunks * (4 / p->wq);
    static const int nt_env = rmu_env("RMU_NT") ? atoi(rmu_env("RMU_NT")) : 1;
    p->nt = (nt_env && p->nqt == 1 && p->kv == 0 && p->wq <= 2) ? 1 : 0;
    p->lds_bytes = with_wcfg(p->wq, p->kv, 0, [](auto c) { return (int)decltype(c)::LDS_BYTES; });
    return p->lds_bytes > 0 ? RMU_OK : RMU_E_INVALID;
}

int rmu_wide_launch(const ScanLaunch* p, hipStream_t s) {
    return with_wcfg(p->wq, p->kv, p->nt, [&](auto c) { return launch_cfg<decltype(c), scan_wide_kernel<decltype(c)>>(p, s); });
}

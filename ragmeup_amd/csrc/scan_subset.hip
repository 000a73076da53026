// scan_subset.hip -- exact fp32 top-k over a SUBSET of the stored rows: a gathered form of scan_topk.hip (gfx950 / MI355X only).
//
// Replaces: the FILTERED similarity search the reference reaches through VectorStore.similarity_search(**kwargs) --
//   Milvus col.search(expr='source == "a.pdf"') / PGVector filter={"source": "a.pdf"} (server/RAGHelper.py:497-499 with search_kwargs).
//
// One ascending list of row ids per call, shared by all its queries.  The work is that of scan_topk_kernel -- query fragments in
// registers, corpus rows HBM -> LDS through a ring of K-chunks filled by LDS-DMA, v_mfma_f32_32x32x2_f32 in the SAME k order (the
// k-permutation and the swizzled LDS image are documented at the head of scan_topk.hip), per-(wave, query) candidate slots in LDS -- so
// every score has the bits rmu_index_search gives the same row.  What differs:
//   * GATHER.  The global address of a global_load_lds is per lane (only the LDS side is lane-linear), so lane f of a DMA instruction
//     reads its 16-byte unit from row ids[tile * RT + i] instead of row tile * RT + i.  A row is contiguous (dpad * 4 bytes), so the
//     gather still moves whole 128-byte lines; nothing is copied anywhere first and the time follows the subset, not the corpus.
//   * ROW IDS.  The int64 list is narrowed once per call to u32 (absent = 0xFFFFFFFF: out of [0, n), or padding up to a whole tile).  A
//     tile's ids reach the lanes by a 4-byte-per-lane LDS-DMA into a per-wave landing zone, issued one ring step before the first chunk
//     of that tile is requested (three before it is computed) and covered by the next counted vmcnt, then ds_read: an ordinary
//     global_load here would make hipcc wait vmcnt(0) and drain the ring.  An absent id is never dereferenced (its lanes read row 0)
//     and its score never passes the filter.
//   * KEYS carry the POSITION in the list.  The list is ascending, so (score, then lower position) is the project's tie rule; the
//     partials go through rmu_merge_final_launch as they are and k_subset_map turns positions into row ids (+ row_base) behind it.
//   * The filter of a tile runs behind its own MFMA chain (no second accumulator): filtered queries are mostly interactive, the ring
//     keeps filling meanwhile.  The shared thresholds are published (compact_slot) but not read.
// Two geometries: WQ = 1 -- 32 queries per workgroup, the four waves on different 32-row slices of a 128-row tile (HBM-bound, k <= 32);
// WQ = 4 -- 128 queries per workgroup, every wave on the same 32-row tile (larger batches, and every k > 32: the 128-deep slots leave no
// room for a 128-row tile).
#include "rmu_common.h"
#include "scan_common.h"
#include "../../include/rmu.h"

namespace {

template <int D_, int WQ_, int CKF_, int CAP_, int NCHECK_>
struct SCfg {
    static constexpr int D = D_;            // padded row length (floats)
    static constexpr int WQ = WQ_;          // query groups per workgroup
    static constexpr int RP = 4 / WQ_;      // row parts per tile
    static constexpr int RT = 32 * RP;      // rows per tile
    static constexpr int CKF = CKF_;        // floats per K-chunk
    static constexpr int U16 = CKF_ / 4;    // 16-byte units per row-chunk
    static constexpr int NCH = D_ / CKF_;   // chunks per tile
    static constexpr int TS = CKF_ / 8;     // ds_read_b128 steps per chunk
    static constexpr int RING = 3;          // two chunks in flight
    static constexpr int SLOT_BYTES = RT * CKF_ * 4;
    static constexpr int NI = RT * U16 / 256;  // DMA wave-instructions per wave per chunk
    static constexpr int IDN = (RT + 63) / 64; // 4-byte DMA wave-instructions per wave per tile (row ids)
    static constexpr int CAP = CAP_;
    static constexpr int NPL = (CAP_ + 63) / 64;
    static constexpr int NCHECK = NCHECK_;
    static constexpr int A = 32 / NCHECK_;  // max appends per slot between overflow checks
    static constexpr int SWB = (U16 % 16 == 8) ? 8 : 4;  // swizzle block (units)
    static constexpr int RING_BYTES = RING * SLOT_BYTES;
    static constexpr int CAND_BYTES = 4 * 32 * CAP_ * 8;
    static constexpr int CNT_OFF = RING_BYTES + CAND_BYTES;
    static constexpr int THR_OFF = CNT_OFF + 4 * 32 * 4;
    static constexpr int TRASH_OFF = THR_OFF + 4 * 32 * 4;   // one private 8-B trash slot per lane
    static constexpr int IDS_OFF = TRASH_OFF + 256 * 8;      // per-wave landing zone of a tile's row ids (128 u32)
    static constexpr int LDS_BYTES = IDS_OFF + 4 * 512;
    static_assert(D_ % CKF_ == 0 && CKF_ % 8 == 0, "chunking");
    static_assert((RT * U16) % 256 == 0, "DMA split");
    static_assert(U16 % 16 == 8 || U16 % 16 == 4 || U16 % 16 == 12, "swizzle classes");
    static_assert(NCH >= 3, "the row ids of a tile are requested three steps and read two steps before its first chunk is computed");
    static_assert(LDS_BYTES <= 160 * 1024, "LDS");
    static_assert(NI + IDN <= 63, "vmcnt field");
};

__device__ __forceinline__ int swz(int row, int swb) { return swb == 8 ? ((row >> 1) & 7) : ((row >> 2) & 3); }

extern __shared__ __attribute__((aligned(16))) char smem[];

template <class C>
__global__ __launch_bounds__(256) void scan_subset_kernel(const SubsetLaunch a) {
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = w % C::WQ;   // query group of this wave
    const int rp = w / C::WQ;  // row part of this wave
    const int h = lane >> 5;
    const int j = lane & 31;

    // ---- block -> (list chunk, query tile), as scan_topk_kernel ------------------------------------
    int s_idx, qt;
    {
        const int b = blockIdx.x;
        if ((a.s_chunks & 7) == 0) {
            const int xcd = b & 7, m = b >> 3;
            qt = m % a.nqt;
            s_idx = (m / a.nqt) * 8 + xcd;
        } else {
            qt = b % a.nqt;
            s_idx = b / a.nqt;
        }
    }
    const int64_t tiles_total = (a.n_sub + C::RT - 1) / C::RT;
    const int64_t t0 = (int64_t)s_idx * a.tiles_per_chunk;
    int64_t t1 = t0 + a.tiles_per_chunk;
    if (t1 > tiles_total) t1 = tiles_total;
    const int ntiles = (int)(t1 > t0 ? t1 - t0 : 0);

    char* ring = smem;
    u64* cand_w = (u64*)(smem + C::RING_BYTES) + (size_t)w * 32 * C::CAP;
    u32* cnt_w = (u32*)(smem + C::CNT_OFF) + w * 32;
    float* thr_w = (float*)(smem + C::THR_OFF) + w * 32;
    const u32* ids_w = (const u32*)(smem + C::IDS_OFF + w * 512);

    const int q_idx = (qt * C::WQ + g) * 32 + j;
    const bool q_ok = q_idx < a.nq;
    if (lane < 32) {
        cnt_w[lane] = 0;
        thr_w[lane] = q_ok ? -INFINITY : INFINITY;
    }
    float thr = q_ok ? -INFINITY : INFINITY;
    u32* gthr_w = a.gthr + (qt * C::WQ + g) * 32;

    // ---- query fragments -> registers (padded query columns read row 0: their threshold is +inf) ---
    f32x4 qf[C::D / 8];
    {
        const float* qrow = a.q + (size_t)(q_ok ? q_idx : 0) * C::D + 4 * h;
#pragma unroll
        for (int t = 0; t < C::D / 8; ++t) qf[t] = *(const f32x4*)(qrow + 8 * t);
    }

    // ---- per-lane DMA map: row of the tile and byte offset of the (de-swizzled) 16-B unit inside that row's chunk --------------
    const u32 n_rows = (u32)a.n_rows;
    const char* src[C::NI];       // this lane's source of chunk 0 of the tile whose chunks are being requested
    auto set_src = [&](int n, u32 id) {
        const int f = (n * 4 + w) * 64 + lane;
        const int i = f / C::U16, p = f % C::U16;
        src[n] = (const char*)a.x + (size_t)(id < n_rows ? id : 0u) * (size_t)(C::D * 4) + (u32)(4 * (p ^ swz(i, C::SWB))) * 4u;
    };
    auto tile_row = [&](int n) { return ((n * 4 + w) * 64 + lane) / C::U16; };
    // validity of the 32 rows of this wave's slice, as the 16 accumulator rows of this lane see them (row (r & 3) + 8 (r >> 2) + 4 h)
    auto lane_valid = [&](u32 id_of_slice_row_j) -> u32 {
        const u32 vm = (u32)__ballot(lane < 32 && id_of_slice_row_j < n_rows) >> (4 * h);
        return (vm & 0xFu) | ((vm >> 4) & 0xF0u) | ((vm >> 8) & 0xF00u) | ((vm >> 12) & 0xF000u);
    };
    auto clamp_tile = [&](int tl) { return t0 + (tl < ntiles ? tl : ntiles - 1); };   // tail: harmless reloads keep the vmcnt bookkeeping uniform
    auto issue_ids = [&](int tl) {
        const u32* s = a.ids + clamp_tile(tl) * C::RT + lane;     // (RT = 32: lanes 32..63 read the next tile's ids; the list is padded)
#pragma unroll
        for (int n = 0; n < C::IDN; ++n)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(s + 64 * n),
                                             (__attribute__((address_space(3))) void*)(smem + C::IDS_OFF + w * 512 + n * 256), 4, 0, 0);
    };
    auto issue_chunk = [&](int c, int slot) {   // chunk c of the tile `src` points at -> ring slot
        char* dst = ring + slot * C::SLOT_BYTES;
#pragma unroll
        for (int n = 0; n < C::NI; ++n)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src[n] + c * C::CKF * 4),
                                             (__attribute__((address_space(3))) void*)(dst + (n * 4 + w) * 1024), 16, 0, 0);
    };

    // A-fragment read offsets: row (32*rp + j), unit (2t+h) ^ swz
    const int rowi = 32 * rp + j;
    int abase[C::SWB / 2];
#pragma unroll
    for (int m = 0; m < C::SWB / 2; ++m)
        abase[m] = (rowi * C::U16 + ((2 * m + h) ^ swz(rowi, C::SWB))) * 16;
    auto read_frag = [&](int slot_off, int t) -> f32x4 {
        const int off = abase[t % (C::SWB / 2)] + (t / (C::SWB / 2)) * (C::SWB * 16);
        return *(const f32x4*)(ring + slot_off + off);
    };

    const u32 cnt_addr = lds_addr(cnt_w + j);
    const u32 cand_addr = lds_addr(cand_w + j * C::CAP);
    const u32 trash_addr = lds_addr(smem + C::TRASH_OFF) + threadIdx.x * 8u;

    auto check_compact = [&]() {
        const u32 c = cnt_w[j];
        const u64 bal = __ballot(c > (u32)(C::CAP - C::A));
        u32 mask = (u32)bal | (u32)(bal >> 32);
        if (mask) {
            while (mask) {
                const int jj = __builtin_ctz(mask);
                mask &= mask - 1;
                compact_slot<C>(jj, cand_w, cnt_w, thr_w, a.k, lane, gthr_w);
            }
            thr = thr_w[j];
        }
    };
    // append the rows of `acc` that pass (pmask) to this lane's query slot.  All LDS writes are inline asm: a compiler-generated LDS
    // write is ordered behind the in-flight LDS-DMA with s_waitcnt vmcnt(0) and would drain the ring (scan_topk.hip).
    auto append_round = [&](const f32x16& acc, u32 pmask, u32 bits, int r0, int r1, u32 pos0) {
        const u32 n = __builtin_popcount(pmask & bits);
        u32 res_pos;
        asm volatile("ds_add_rtn_u32 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=v"(res_pos) : "v"(cnt_addr), "v"(n) : "memory");
        u32 wr_addr = cand_addr + res_pos * 8u;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (r < r0 || r >= r1) continue;
            const u64 key = rmu_make_key(acc[r] + 0.0f, pos0 + (u32)((r & 3) + 8 * (r >> 2)));
            const bool pass = (pmask >> r) & 1u;
            lds_store_b64_nofence(pass ? wr_addr : trash_addr, key);   // every lane stores, the non-passing ones into their trash slot
            wr_addr += pass ? 8u : 0u;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        check_compact();
    };

    if (ntiles > 0) {
        // ---- prologue: tile 0's ids by ordinary loads (nothing is in flight yet), RING-1 chunks requested ---------------------------
        u32 valid_cur, valid_nxt = 0;
        {
            const u32* ids0 = a.ids + t0 * C::RT;
#pragma unroll
            for (int n = 0; n < C::NI; ++n) set_src(n, ids0[tile_row(n)]);
            valid_cur = lane_valid(ids0[rowi]);
        }
        issue_chunk(0, 0);
        issue_chunk(1, 1);
        int slot = 0, islot = 2;     // ring slot of the chunk computed / requested in this step
        for (int tl = 0; tl < ntiles; ++tl) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
            for (int c = 0; c < C::NCH; ++c) {
                // own DMA of this chunk (and of everything older, row ids included) has landed; own LDS reads have returned
                asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(C::NI) : "memory");
                __builtin_amdgcn_s_barrier();
                if (c == C::NCH - 3) issue_ids(tl + 1);       // covered by the counted wait of the next step
                if (c == C::NCH - 2) {                        // the next tile's first chunk is requested below: its ids -> addresses
#pragma unroll
                    for (int n = 0; n < C::NI; ++n) set_src(n, ids_w[tile_row(n)]);
                    valid_nxt = lane_valid(ids_w[rowi]);
                }
                issue_chunk((c + 2) % C::NCH, islot);         // refills the slot every wave finished reading last step
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
            // ---- filter of this tile: absent and tombstoned (NaN) rows never pass ------------------------------------------------
            u32 pmask = 0;
#pragma unroll
            for (int r = 0; r < 16; ++r) pmask |= (acc[r] > thr) ? (1u << r) : 0u;
            pmask &= valid_cur;
            if (__any(pmask != 0)) {
                const u32 pos0 = (u32)((t0 + tl) * C::RT) + (u32)(32 * rp + 4 * h);
                if (C::NCHECK == 2) {
                    append_round(acc, pmask, 0x00FFu, 0, 8, pos0);
                    append_round(acc, pmask, 0xFF00u, 8, 16, pos0);
                } else {
                    append_round(acc, pmask, 0xFFFFu, 0, 16, pos0);
                }
            }
            valid_cur = valid_nxt;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }

    // ---- final: sort every slot, emit k keys per (part, query) ---------------------------------------
    const int part = s_idx * C::RP + rp;
    for (int jj = 0; jj < 32; ++jj) {
        const int qq = (qt * C::WQ + g) * 32 + jj;
        if (qq >= a.nq) break;
        const u32 n = cnt_w[jj];
        u64 key[C::NPL];
        u32 rank[C::NPL];
#pragma unroll
        for (int p = 0; p < C::NPL; ++p) {
            const u32 e = lane + 64 * p;
            key[p] = (e < n) ? cand_w[jj * C::CAP + e] : 0ull;
        }
        rank_keys<C::NPL>(key, n, rank);
        u64* dst = a.partial + ((size_t)part * a.nq + qq) * a.k;
#pragma unroll
        for (int p = 0; p < C::NPL; ++p) {
            const u32 e = lane + 64 * p;
            if (e < n) {
                if (rank[p] < (u32)a.k) dst[rank[p]] = key[p];
            } else if (e < (u32)a.k) {
                dst[e] = 0ull;   // fewer than k candidates: pad (e >= n are exactly the unfilled ranks)
            }
        }
    }
}

// int64 list -> u32 ids, absent = 0xFFFFFFFF (outside [0, n_rows), or the padding past n_sub)
__global__ void k_subset_narrow(const int64_t* __restrict__ rows, int64_t n_sub, int64_t n_rows, u32* __restrict__ ids, int64_t n_pad) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pad) return;
    u32 v = 0xFFFFFFFFu;
    if (i < n_sub) {
        const int64_t r = rows[i];
        if (r >= 0 && r < n_rows) v = (u32)r;
    }
    ids[i] = v;
}

// merged positions -> row ids (+ row_base); -1 stays -1
__global__ void k_subset_map(int64_t* __restrict__ out_rows, const u32* __restrict__ ids, int64_t total, int64_t row_base) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t p = out_rows[i];
    out_rows[i] = p >= 0 ? (int64_t)ids[p] + row_base : -1;
}

template <class C>
int launch_cfg(const SubsetLaunch* p, hipStream_t s) {
    static const hipError_t attr_rc =
        hipFuncSetAttribute((const void*)scan_subset_kernel<C>, hipFuncAttributeMaxDynamicSharedMemorySize, C::LDS_BYTES);
    if (attr_rc != hipSuccess) return RMU_E_HIP;
    hipLaunchKernelGGL(scan_subset_kernel<C>, dim3(p->grid), dim3(256), C::LDS_BYTES, s, *p);
    return hipGetLastError() == hipSuccess ? RMU_OK : RMU_E_HIP;
}

// geometry table: (WQ) x (k class).  kv 0: k <= 32 (CAP 64, one check per tile); kv 1: k <= 112 (CAP 128, two).
//                                     D   WQ  CKF      CAP NCHECK
template <int D> using S_w1_k0 = SCfg<D, 1, 48, 64, 1>;                   // 72 KiB ring (48 KiB in flight) + 64 KiB candidates
template <int D> using S_w4_k0 = SCfg<D, 4, D == 192 ? 32 : 96, 64, 1>;   // 36 KiB ring (192-wide rows: 12 KiB, six chunks per tile)
template <int D> using S_w4_k1 = SCfg<D, 4, 32, 128, 2>;                  // 12 KiB ring + 128 KiB candidates

template <int D>
int launch_d(const SubsetLaunch* p, hipStream_t s) {
    switch (p->wq * 2 + p->kv) {
        case 2: return launch_cfg<S_w1_k0<D>>(p, s);
        case 8: return launch_cfg<S_w4_k0<D>>(p, s);
        case 9: return launch_cfg<S_w4_k1<D>>(p, s);
        default: return RMU_E_INVALID;
    }
}
template <int D>
int lds_d(int wq, int kv) {
    switch (wq * 2 + kv) {
        case 2: return S_w1_k0<D>::LDS_BYTES;
        case 8: return S_w4_k0<D>::LDS_BYTES;
        case 9: return S_w4_k1<D>::LDS_BYTES;
        default: return -1;
    }
}

}  // namespace

int64_t rmu_subset_ids_len(int64_t n_sub) { return (n_sub + 127) / 128 * 128 + 128; }

int rmu_subset_plan(SubsetLaunch* p) {
    if (p->k < 1 || p->k > RMU_MAX_K || p->nq < 1 || p->n_sub < 0 || p->n_rows < 1 || p->n_rows >= 0xFFFFFFFFll || p->n_sub >= 0xFFFFFFFFll)
        return RMU_E_INVALID;
    if (p->dpad != 192 && p->dpad != 384 && p->dpad != 768) return RMU_E_INVALID;
    p->kv = p->k <= 32 ? 0 : 1;
    p->wq = (p->nq <= 32 && p->kv == 0) ? 1 : 4;
    const int rt = 32 * (4 / p->wq);
    p->nqt = (p->nq + 32 * p->wq - 1) / (32 * p->wq);
    const int64_t tiles_total = (p->n_sub + rt - 1) / rt;
    // list chunks: a multiple of 8 (XCD-aware block map) that makes grid = S*nqt fill 256 CUs evenly (as rmu_scan_plan)
    int best_s = 8;
    double best_eff = -1.0;
    for (int s = 8; s <= 256; s += 8) {
        const int64_t total = (int64_t)s * p->nqt;
        const double eff = (double)total / (double)(((total + 255) / 256) * 256);
        if (eff > best_eff + 1e-9) { best_eff = eff; best_s = s; }
        if (total >= 256 && eff > 0.999) break;
    }
    int s = best_s;
    if (tiles_total < s) s = tiles_total > 0 ? (int)tiles_total : 1;
    p->tiles_per_chunk = (int)((tiles_total + s - 1) / s);
    if (p->tiles_per_chunk < 1) p->tiles_per_chunk = 1;
    const int64_t used = (tiles_total + p->tiles_per_chunk - 1) / p->tiles_per_chunk;
    if (used > 0 && used < s) s = (int)used;
    p->s_chunks = s;
    p->grid = s * p->nqt;
    p->parts = s * (4 / p->wq);
    p->lds_bytes = p->dpad == 384 ? lds_d<384>(p->wq, p->kv) : p->dpad == 768 ? lds_d<768>(p->wq, p->kv) : lds_d<192>(p->wq, p->kv);
    return p->lds_bytes > 0 ? RMU_OK : RMU_E_INVALID;
}

int rmu_subset_launch(const SubsetLaunch* p, hipStream_t s) {
    switch (p->dpad) {
        case 384: return launch_d<384>(p, s);
        case 768: return launch_d<768>(p, s);
        case 192: return launch_d<192>(p, s);
        default: return RMU_E_INVALID;
    }
}

int rmu_subset_narrow_launch(const int64_t* rows, int64_t n_sub, int64_t n_rows, u32* ids, hipStream_t s) {
    const int64_t n_pad = rmu_subset_ids_len(n_sub);
    hipLaunchKernelGGL(k_subset_narrow, dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0, s, rows, n_sub, n_rows, ids, n_pad);
    return hipGetLastError() == hipSuccess ? RMU_OK : RMU_E_HIP;
}

int rmu_subset_map_launch(int64_t* out_rows, const u32* ids, int64_t total, int64_t row_base, hipStream_t s) {
    hipLaunchKernelGGL(k_subset_map, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, out_rows, ids, total, row_base);
    return hipGetLastError() == hipSuccess ? RMU_OK : RMU_E_HIP;
}

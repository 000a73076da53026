// scan_subset.hip -- exact fp32 top-k over a SUBSET of the stored rows: a gathered form of scan_topk.hip (gfx950 / MI355X only).
//
// Replaces: the FILTERED similarity search the reference reaches through VectorStore.similarity_search(**kwargs) --
//   Milvus col.search(expr='source == "a.pdf"') / PGVector filter={"source": "a.pdf"} (server/RAGHelper.py:497-499 with search_kwargs).
//
// One ascending list of row ids per call, shared by all its queries (scan_subset_kernel, rmu_index_search_subset), or one list per group of
// adjacent queries, every group in one launch (scan_groups_kernel behind rmu_groups_plan's work table, rmu_index_search_groups): two
// __global__s over ONE tile loop (subset_scan).  Every score has the bits rmu_index_search gives the same row
// because both kernels are built from the SAME pieces of scan_common.h: the geometry (ScanGeom) and the swizzle of the LDS image, the
// block map, the A-fragment reads (afrag_base, afrag_read), the per-(wave, query) candidate slots in LDS (carve_slots, compact_slot) and
// the final emit (emit_slots).  The query fragments sit in registers and the MFMA chain below issues v_mfma_f32_32x32x2_f32 in the k order
// documented at the head of scan_topk.hip.  What is this file's own -- the tile loop:
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

// RING = 3: two chunks in flight
template <int D_, int WQ_, int CKF_, int CAP_, int NCHECK_>
struct SCfg : ScanGeom<D_, WQ_, CKF_, 3, CAP_, NCHECK_> {
    using G = ScanGeom<D_, WQ_, CKF_, 3, CAP_, NCHECK_>;
    static constexpr int IDN = (G::RT + 63) / 64;            // 4-byte DMA wave-instructions per wave per tile (row ids)
    static constexpr int IDS_OFF = G::TAIL_OFF;              // per-wave landing zone of a tile's row ids (128 u32)
    static constexpr int LDS_BYTES = IDS_OFF + 4 * 512;
    static_assert(G::NCH >= 3, "the row ids of a tile are requested three steps and read two steps before its first chunk is computed");
    static_assert(LDS_BYTES <= 160 * 1024, "LDS");
    static_assert(G::NI + IDN <= 63, "vmcnt field");
};

extern __shared__ __attribute__((aligned(16))) char smem[];

// what a launch of either kernel holds for all its workgroups (SubsetLaunch and GroupsLaunch both fill one)
struct SubsetArgs {
    const float* x; u32 n_rows; const float* q; int nq /* stride of `partial` */; int k; u64* partial; u32* gthr;
};

// The tile loop, ONE copy for scan_subset_kernel (one list per launch) and scan_groups_kernel (one list per group of queries): the grouped
// form's scores and order are the ungrouped form's by construction.  A workgroup scans tiles [t0, t0 + ntiles) of the list whose narrowed
// ids start at `ids` for the 32 * WQ queries from q_first on, of which those below q_end are its own (q_first is ANY query index in the
// grouped form: the lanes from q_end on are padding, they keep a +inf threshold, never append and are not emitted, although their indices
// belong to the next group), and emits parts part0 .. part0 + RP - 1.  Key positions count from the start of the list.  All of these are
// wave-uniform.
template <class C>
__device__ __forceinline__ void subset_scan(const SubsetArgs& a, const u32* ids, int64_t t0, int ntiles, int q_first, int q_end, int part0) {
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = w % C::WQ;   // query group of this wave
    const int rp = w / C::WQ;  // row part of this wave
    const int h = lane >> 5;
    const int j = lane & 31;

    char* ring = smem;
    const u32* ids_w = (const u32*)(smem + C::IDS_OFF + w * 512);

    const int q_base = q_first + g * 32, q_idx = q_base + j;
    const bool q_ok = q_idx < q_end;
    u64* cand_w;
    u32* cnt_w;
    float* thr_w;
    carve_slots<C>(smem, w, lane, q_ok, cand_w, cnt_w, thr_w);
    float thr = q_ok ? -INFINITY : INFINITY;
    u32* gthr_w = a.gthr + q_base;

    // ---- query fragments -> registers, as scan_topk_kernel (padded query columns read row 0: their threshold is +inf).  One copy per
    // kernel: see the head of scan_common.h -------------------------------------------------------------------------------------------
    f32x4 qf[C::D / 8];
    {
        const float* qrow = a.q + (size_t)(q_ok ? q_idx : 0) * C::D + 4 * h;
#pragma unroll
        for (int t = 0; t < C::D / 8; ++t) qf[t] = *(const f32x4*)(qrow + 8 * t);
    }

    // ---- per-lane DMA map: row of the tile and byte offset of the (de-swizzled) 16-B unit inside that row's chunk --------------
    const u32 n_rows = a.n_rows;
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
        const u32* s = ids + clamp_tile(tl) * C::RT + lane;     // (RT = 32: lanes 32..63 read the next tile's ids; the list is padded)
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

    const int rowi = 32 * rp + j;
    int abase[C::SWB / 2];
#pragma unroll
    for (int m = 0; m < C::SWB / 2; ++m) abase[m] = afrag_base<C>(rowi, h, m);
    auto read_frag = [&](int slot_off, int t) -> f32x4 { return afrag_read<C>(ring, abase, slot_off, t); };

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
            append_key(pass, wr_addr, trash_addr, key);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        check_compact();
    };

    if (ntiles > 0) {
        // ---- prologue: tile 0's ids by ordinary loads (nothing is in flight yet), RING-1 chunks requested ---------------------------
        u32 valid_cur, valid_nxt = 0;
        {
            const u32* ids0 = ids + t0 * C::RT;
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

    emit_slots<C>(cand_w, cnt_w, a.partial, part0 + rp, q_base, q_end, a.nq, a.k, lane);
}

template <class C>
__global__ __launch_bounds__(256) void scan_subset_kernel(const SubsetLaunch a) {
    int s_idx, qt;   // list chunk, query tile
    block_map(a.s_chunks, a.nqt, s_idx, qt);
    const int64_t tiles_total = (a.n_sub + C::RT - 1) / C::RT;
    const int64_t t0 = (int64_t)s_idx * a.tiles_per_chunk;
    int64_t t1 = t0 + a.tiles_per_chunk;
    if (t1 > tiles_total) t1 = tiles_total;
    const int ntiles = (int)(t1 > t0 ? t1 - t0 : 0);
    const SubsetArgs sa{a.x, (u32)a.n_rows, a.q, a.nq, a.k, a.partial, a.gthr};
    subset_scan<C>(sa, a.ids, t0, ntiles, qt * C::WQ * 32, a.nq, s_idx * C::RP);
}

// One list per group of queries (rmu_index_search_groups): workgroup b takes descriptor b of the table rmu_groups_plan wrote -- uniform
// values, fetched once here -- and runs the same tile loop.  A null descriptor (ntiles = 0, q_end = 0: the padding that keeps the XCD
// order of the table) scans and emits nothing.
template <class C>
__global__ __launch_bounds__(256) void scan_groups_kernel(const GroupsLaunch a) {
    const GroupDesc d = a.tab[blockIdx.x];
    const SubsetArgs sa{a.x, (u32)a.n_rows, a.q, a.nq, a.k, a.partial, a.gthr};
    subset_scan<C>(sa, a.ids + d.ids_off, (int64_t)d.t0, (int)d.ntiles, (int)d.q_first, (int)d.q_end, (int)d.part0);
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

// the grouped form of the two kernels above.  Entry i of the narrowed ids belongs to the last list whose ids_off is <= i
__global__ void k_groups_narrow(const int64_t* __restrict__ rows, const GroupList* __restrict__ lists, int n_lists, int64_t n_rows,
                                u32* __restrict__ ids, int64_t ids_total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ids_total) return;
    int lo = 0, hi = n_lists - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((int64_t)lists[mid].ids_off <= i) lo = mid; else hi = mid - 1;
    }
    const GroupList l = lists[lo];
    const int64_t j = i - (int64_t)l.ids_off;
    u32 v = 0xFFFFFFFFu;
    if (j < (int64_t)l.len) {
        const int64_t r = rows[l.src + j];
        if (r >= 0 && r < n_rows) v = (u32)r;
    }
    ids[i] = v;
}

// merged positions (inside the query's own list) -> row ids (+ row_base); -1 stays -1
__global__ void k_groups_map(int64_t* __restrict__ out_rows, const u32* __restrict__ ids, const u32* __restrict__ q_off, int64_t total, int k,
                             int64_t row_base) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t p = out_rows[i];
    out_rows[i] = p >= 0 ? (int64_t)ids[(int64_t)q_off[i / k] + p] + row_base : -1;
}

// geometry table: (WQ) x (k class).  kv 0: k <= 32 (CAP 64, one check per tile); kv 1: k <= 112 (CAP 128, two).
//                                     D   WQ  CKF      CAP NCHECK
template <int D> using S_w1_k0 = SCfg<D, 1, 48, 64, 1>;                   // 72 KiB ring (48 KiB in flight) + 64 KiB candidates
template <int D> using S_w4_k0 = SCfg<D, 4, D == 192 ? 32 : 96, 64, 1>;   // 36 KiB ring (192-wide rows: 12 KiB, six chunks per tile)
template <int D> using S_w4_k1 = SCfg<D, 4, 32, 128, 2>;                  // 12 KiB ring + 128 KiB candidates

// (wq, kv) of width D -> f(configuration)
template <int D, class F>
int with_cfg(int wq, int kv, F&& f) {
    switch (wq * 2 + kv) {
        case 2: return f(S_w1_k0<D>{});
        case 8: return f(S_w4_k0<D>{});
        case 9: return f(S_w4_k1<D>{});
        default: return RMU_E_INVALID;
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
    // list chunks as the corpus chunks of rmu_scan_plan
    rmu_plan_chunks(p->nqt, (p->n_sub + rt - 1) / rt, &p->s_chunks, &p->tiles_per_chunk);
    p->grid = p->s_chunks * p->nqt;
    p->parts = p->s_chunks * (4 / p->wq);
    p->lds_bytes = for_dpad(p->dpad, [&](auto d) { return with_cfg<decltype(d)::value>(p->wq, p->kv, [](auto c) { return (int)decltype(c)::LDS_BYTES; }); });
    return p->lds_bytes > 0 ? RMU_OK : RMU_E_INVALID;
}

int rmu_subset_launch(const SubsetLaunch* p, hipStream_t s) {
    return for_dpad(p->dpad, [&](auto d) {
        return with_cfg<decltype(d)::value>(p->wq, p->kv, [&](auto c) { return launch_cfg<decltype(c), scan_subset_kernel<decltype(c)>>(p, s); });
    });
}

// ---- planner of the grouped form.  q_list is non-decreasing, so a GROUP is a run of adjacent queries with one list.
// Geometry per group: rmu_subset_plan's rule (wq = 1 for <= 32 queries and k <= 32, otherwise 4), so a call has at most two classes and two
//   scan launches.  A group of nqt query tiles over T tiles of its list is T * nqt tile-units of work (a tile is 128 rows x 32 queries or
//   32 rows x 128 queries: the same MFMA work either way).
// Rule: with W = the tile-units of the whole call, a workgroup gets at most tpw = ceil(W / 256) tiles: group g is cut into
//   c_g = min(ceil(T_g / tpw), Pcap / RP_g) chunks of ceil(T_g / c_g) tiles (RP = 4 / wq row parts per chunk), every chunk as nqt_g
//   workgroups.  Workgroups: sum c_g nqt_g <= 256 + sum nqt_g (one 256-CU wave and at most one short chunk per group); none is longer
//   than tpw tiles unless Pcap bites.
// Bound: P = max c_g RP_g <= Pcap = min(1024, max(4, 2^25 / (nq k))), so the zeroed partial workspace [P, nq, k] stays within 256 MiB
//   (k <= 112 and nq <= 8192 leave Pcap >= 36; up to 32 768 result slots it is 1024, the most rmu_subset_plan gives one list -- 256 chunks
//   of four row parts -- and the most merge_select_kernel takes).  P is large only while there are few groups: c_g follows T_g / tpw.
// Order of a class's table (DERIVED from the dispatch rule -- consecutive workgroup ids go round-robin over the 8 XCDs -- not measured):
//   the nqt workgroups of one list chunk read the same rows, so they are given ids with the same residue mod 8 and share one XCD's L2.
//   Chunks are dealt to the XCD with the fewest workgroups so far; the table is 8 * (the longest XCD's count) long, shorter XCDs are
//   filled up with null descriptors.
int rmu_groups_plan(int dpad, int k, int nq, const int64_t* list_ptr, const int32_t* q_list, GroupsPlan* out) {
    if (k < 1 || k > RMU_MAX_K || nq < 1) return RMU_E_INVALID;
    if (dpad != 192 && dpad != 384 && dpad != 768) return RMU_E_INVALID;
    const int kv = k <= 32 ? 0 : 1;
    struct Grp { int q0, cnt, cls, nqt; int64_t tiles; u32 ids_off; };
    std::vector<Grp> grps;
    out->q_off.assign((size_t)nq, 0u);
    int64_t work = 0;
    for (int q0 = 0; q0 < nq;) {
        int q1 = q0 + 1;
        while (q1 < nq && q_list[q1] == q_list[q0]) ++q1;
        const int64_t src = list_ptr[q_list[q0]], len = list_ptr[q_list[q0] + 1] - src;
        if (len > 0) {                                   // (an empty list: no workgroup, its queries' zeroed partials come out as padding)
            Grp g;
            g.q0 = q0; g.cnt = q1 - q0;
            g.cls = (g.cnt <= 32 && kv == 0) ? 0 : 1;
            const int wq = g.cls ? 4 : 1, rt = 32 * (4 / wq);
            g.nqt = (g.cnt + 32 * wq - 1) / (32 * wq);
            g.tiles = (len + rt - 1) / rt;
            g.ids_off = (u32)out->ids_total;
            out->lists.push_back(GroupList{src, (u32)len, g.ids_off});
            out->ids_total += rmu_subset_ids_len(len);
            if (out->ids_total >= 0x100000000ll) return RMU_E_INVALID;
            for (int i = q0; i < q1; ++i) out->q_off[i] = g.ids_off;
            work += g.tiles * g.nqt;
            grps.push_back(g);
        }
        q0 = q1;
    }
    const int64_t tpw = work > 256 ? (work + 255) / 256 : 1;
    const int64_t slots = (int64_t)nq * k;
    int pcap = (int)((1ll << 25) / slots);
    pcap = pcap > 1024 ? 1024 : (pcap < 4 ? 4 : pcap);
    out->parts = 1;
    std::vector<GroupDesc> per_xcd[2][8];
    for (const Grp& g : grps) {
        const int wq = g.cls ? 4 : 1, rp = 4 / wq;
        int64_t c = (g.tiles + tpw - 1) / tpw;
        if (c > pcap / rp) c = pcap / rp;
        const int64_t tpc = (g.tiles + c - 1) / c;
        c = (g.tiles + tpc - 1) / tpc;                   // (no empty trailing chunk)
        if ((int)c * rp > out->parts) out->parts = (int)c * rp;
        for (int64_t ch = 0; ch < c; ++ch) {
            int xcd = 0;
            for (int x = 1; x < 8; ++x)
                if (per_xcd[g.cls][x].size() < per_xcd[g.cls][xcd].size()) xcd = x;
            const int64_t t0 = ch * tpc, t1 = t0 + tpc < g.tiles ? t0 + tpc : g.tiles;
            for (int qt = 0; qt < g.nqt; ++qt)
                per_xcd[g.cls][xcd].push_back(GroupDesc{g.ids_off, (u32)t0, (u32)(t1 - t0), (u32)(g.q0 + qt * 32 * wq), (u32)(g.q0 + g.cnt),
                                                        (u32)(ch * rp), {0u, 0u}});
        }
    }
    for (int cls = 0; cls < 2; ++cls) {
        size_t longest = 0;
        for (int x = 0; x < 8; ++x) longest = per_xcd[cls][x].size() > longest ? per_xcd[cls][x].size() : longest;
        out->tab[cls].assign(longest * 8, GroupDesc{0u, 0u, 0u, 0u, 0u, 0u, {0u, 0u}});
        for (int x = 0; x < 8; ++x)
            for (size_t m = 0; m < per_xcd[cls][x].size(); ++m) out->tab[cls][m * 8 + x] = per_xcd[cls][x][m];
        out->lds_bytes[cls] = for_dpad(dpad, [&](auto d) { return with_cfg<decltype(d)::value>(cls ? 4 : 1, cls ? kv : 0, [](auto c) { return (int)decltype(c)::LDS_BYTES; }); });
        if (out->lds_bytes[cls] <= 0) return RMU_E_INVALID;
    }
    return RMU_OK;
}

int rmu_groups_launch(const GroupsLaunch* p, hipStream_t s) {
    return for_dpad(p->dpad, [&](auto d) {
        return with_cfg<decltype(d)::value>(p->wq, p->kv, [&](auto c) { return launch_cfg<decltype(c), scan_groups_kernel<decltype(c)>>(p, s); });
    });
}

int rmu_groups_narrow_launch(const int64_t* rows, const GroupList* lists, int n_lists, int64_t n_rows, u32* ids, int64_t ids_total, hipStream_t s) {
    hipLaunchKernelGGL(k_groups_narrow, dim3((unsigned)((ids_total + 255) / 256)), dim3(256), 0, s, rows, lists, n_lists, n_rows, ids, ids_total);
    return hipGetLastError() == hipSuccess ? RMU_OK : RMU_E_HIP;
}

int rmu_groups_map_launch(int64_t* out_rows, const u32* ids, const u32* q_off, int64_t total, int k, int64_t row_base, hipStream_t s) {
    hipLaunchKernelGGL(k_groups_map, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, out_rows, ids, q_off, total, k, row_base);
    return hipGetLastError() == hipSuccess ? RMU_OK : RMU_E_HIP;
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

// scan_common.h -- what the scan kernels share.
//   All three (scan_topk.hip, scan_subset.hip, scan_screen.hip): the XCD-aware block map, LDS stores that do not drain the LDS-DMA ring,
//     the enumeration sort, launch_cfg.
//   The exact fp32 scan (scan_topk.hip) and its gathered form (scan_subset.hip), whose scores must agree bit for bit, hold ONE copy of
//     the geometry (ScanGeom), the swizzle, the A-fragment addresses and reads, the candidate slots in LDS (carve, compaction, final
//     emit), the two steps of the append protocol that need no kernel state (append_key, full_slots) and the dispatch over the padded
//     widths.  Their tile loops -- how a chunk's addresses are formed, where the filter runs, the reserve / wait statements of the append
//     protocol and the cycle counters between them -- stay in their own files, and so does the load of the query fragments (eight
//     lines in each): every shared form of it tried (array by reference, by pointer, returned in a struct, the address alone) changed
//     hipcc's register allocation inside the tile loop of SCfg<192, 1, 48, 64, 1>.
#pragma once
#include <type_traits>
#include "rmu_common.h"
#include "../../include/rmu.h"

namespace {

// LDS byte address of a pointer into dynamic shared memory
__device__ __forceinline__ u32 lds_addr(const void* p) {
    return (u32)(uintptr_t)(__attribute__((address_space(3))) char*)(char*)p;
}
// LDS stores as inline asm: a compiler-generated LDS write is ordered behind the in-flight LDS-DMA with
// s_waitcnt vmcnt(0) and would drain the ring.
__device__ __forceinline__ void lds_store_b64(u32 addr, u64 v) {
    asm volatile("ds_write_b64 %0, %1" ::"v"(addr), "v"(v) : "memory");
}
// same, without the "memory" clobber: the compiler may move its own ring reads across it (the targets never
// alias the ring); a clobbering wait follows before anything reads the stored data back
__device__ __forceinline__ void lds_store_b64_nofence(u32 addr, u64 v) {
    asm volatile("ds_write_b64 %0, %1" ::"v"(addr), "v"(v));
}
__device__ __forceinline__ void lds_store_b32(u32 addr, u32 v) {
    asm volatile("ds_write_b32 %0, %1" ::"v"(addr), "v"(v) : "memory");
}

// rank[p] = number of the wave's n keys that are larger than key[p]  (keys are distinct or 0).
// Enumeration sort: broadcast key i with v_readlane (no LDS traffic), every lane counts.  ~6 instructions
// per candidate; a compaction runs while the other three waves of the workgroup wait at the ring barrier,
// so its latency is paid four times -- the shuffle bitonic sort used here before cost 10% of the kernel.
template <int NPL>
__device__ __forceinline__ void rank_keys(const u64 (&key)[NPL], u32 n, u32 (&rank)[NPL]) {
#pragma unroll
    for (int p = 0; p < NPL; ++p) rank[p] = 0;
#pragma unroll
    for (int sp = 0; sp < NPL; ++sp) {
        const u32 lim = n > 64u * sp ? (n - 64u * sp < 64u ? n - 64u * sp : 64u) : 0u;
        const u32 lo = (u32)key[sp], hi = (u32)(key[sp] >> 32);
        // (round 6) four candidates per trip: one candidate is a chain readlane -> SGPR pair -> 64-bit compare -> VCC -> add, ~90 cycles when the
        // wave is alone on its SIMD (the emit of a cold range: 32 queries x 32 candidates = 1.6 us per query); four independent chains overlap
        u32 i = 0;
        for (; i + 4 <= lim; i += 4) {
            u64 ki[4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                ki[u] = ((u64)(u32)__builtin_amdgcn_readlane((int)hi, (int)(i + u)) << 32) | (u64)(u32)__builtin_amdgcn_readlane((int)lo, (int)(i + u));
#pragma unroll
            for (int p = 0; p < NPL; ++p) {
                u32 c[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) c[u] = (ki[u] > key[p]) ? 1u : 0u;
                rank[p] += (c[0] + c[1]) + (c[2] + c[3]);
            }
        }
        for (; i < lim; ++i) {
            const u64 ki = ((u64)(u32)__builtin_amdgcn_readlane((int)hi, (int)i) << 32) |
                           (u64)(u32)__builtin_amdgcn_readlane((int)lo, (int)i);
#pragma unroll
            for (int p = 0; p < NPL; ++p) rank[p] += (ki > key[p]) ? 1u : 0u;
        }
    }
}

// keep the best k of slot j (sorted, best first), refresh its threshold and count
template <class C>
__device__ __forceinline__ void compact_slot(int j, u64* cand_w, u32* cnt_w, float* thr_w, int k, int lane,
                                             u32* gthr_w /* global, this wave's 32 queries */) {
    const u32 n_raw = cnt_w[j];
    const u32 n = n_raw < (u32)C::CAP ? n_raw : (u32)C::CAP;   // the screening scan lets the count run past a full slot
    u64 key[C::NPL];
    u32 rank[C::NPL];
#pragma unroll
    for (int p = 0; p < C::NPL; ++p) {
        const u32 e = lane + 64 * p;
        key[p] = (e < n) ? cand_w[j * C::CAP + e] : 0ull;
    }
    rank_keys<C::NPL>(key, n, rank);
    const u32 base = lds_addr(cand_w + j * C::CAP);
#pragma unroll
    for (int p = 0; p < C::NPL; ++p) {
        const u32 e = lane + 64 * p;
        if (e < n && rank[p] < (u32)k) {
            lds_store_b64(base + rank[p] * 8u, key[p]);
            if (rank[p] == (u32)(k - 1)) {
                lds_store_b32(lds_addr(thr_w + j), __float_as_uint(rmu_key_score(key[p])));
                // publish: this chunk's k-th best is a lower bound of the query's global k-th best
                __hip_atomic_fetch_max(gthr_w + j, (u32)(key[p] >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    if (lane == 0) lds_store_b32(lds_addr(cnt_w + j), n < (u32)k ? n : (u32)k);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// ---- geometry shared by scan_topk_kernel (Cfg) and scan_subset_kernel (SCfg) -----------------------------------------------------
// LDS: [ring][candidate slots][counts][thresholds][trash] and, from TAIL_OFF on, what the deriving configuration adds.
template <int D_, int WQ_, int CKF_, int RING_, int CAP_, int NCHECK_>
struct ScanGeom {
    static constexpr int D = D_;            // padded row length (floats)
    static constexpr int WQ = WQ_;          // query groups per workgroup
    static constexpr int RP = 4 / WQ_;      // row parts per tile
    static constexpr int RT = 32 * RP;      // rows per tile
    static constexpr int CKF = CKF_;        // floats per K-chunk
    static constexpr int U16 = CKF_ / 4;    // 16-byte units per row-chunk
    static constexpr int NCH = D_ / CKF_;   // chunks per tile
    static constexpr int TS = CKF_ / 8;     // ds_read_b128 steps per chunk
    static constexpr int RING = RING_;
    static constexpr int SLOT_BYTES = RT * CKF_ * 4;
    static constexpr int NI = RT * U16 / 256;  // DMA wave-instructions per wave per chunk
    static constexpr int CAP = CAP_;
    static constexpr int NPL = (CAP_ + 63) / 64;
    static constexpr int NCHECK = NCHECK_;
    static constexpr int A = 32 / NCHECK_;  // max appends per slot between overflow checks
    static constexpr int SWB = (U16 % 16 == 8) ? 8 : 4;  // swizzle block (units)
    static constexpr int RING_BYTES = RING_ * SLOT_BYTES;
    static constexpr int CAND_BYTES = 4 * 32 * CAP_ * 8;
    static constexpr int CNT_OFF = RING_BYTES + CAND_BYTES;
    static constexpr int THR_OFF = CNT_OFF + 4 * 32 * 4;
    static constexpr int TRASH_OFF = THR_OFF + 4 * 32 * 4;   // one private 8-B trash slot per lane
    static constexpr int TAIL_OFF = TRASH_OFF + 256 * 8;
    static_assert(D_ % CKF_ == 0 && CKF_ % 8 == 0, "chunking");
    static_assert((RT * U16) % 256 == 0, "DMA split");
    static_assert(U16 % 16 == 8 || U16 % 16 == 4 || U16 % 16 == 12, "swizzle classes");
};

// LDS image of a chunk: the 16-byte unit index is XOR-swizzled by the row (scan_topk.hip header)
__device__ __forceinline__ int swz(int row, int swb) { return swb == 8 ? ((row >> 1) & 7) : ((row >> 2) & 3); }

// block -> (row chunk, query tile); query tiles of one chunk share an XCD's L2
__device__ __forceinline__ void block_map(int s_chunks, int nqt, int& s_idx, int& qt) {
    const int b = blockIdx.x;
    if ((s_chunks & 7) == 0) {
        const int xcd = b & 7, m = b >> 3;
        qt = m % nqt;
        s_idx = (m / nqt) * 8 + xcd;
    } else {
        qt = b % nqt;
        s_idx = b / nqt;
    }
}

// this wave's candidate slots, counts and thresholds in LDS (one object: see guide "three .s-level traps" (a)); empty slots, and a
// threshold nothing passes for the padded query columns
template <class C>
__device__ __forceinline__ void carve_slots(char* smem, int w, int lane, bool q_ok, u64*& cand_w, u32*& cnt_w, float*& thr_w) {
    cand_w = (u64*)(smem + C::RING_BYTES) + (size_t)w * 32 * C::CAP;
    cnt_w = (u32*)(smem + C::CNT_OFF) + w * 32;
    thr_w = (float*)(smem + C::THR_OFF) + w * 32;
    if (lane < 32) {
        cnt_w[lane] = 0;
        thr_w[lane] = q_ok ? -INFINITY : INFINITY;
    }
}

// A-fragment reads of one lane.  Byte offset, inside a chunk's LDS image, of unit (2m + h) ^ swz of row rowi: the lane's read base of
// every step t with t % (SWB / 2) == m ...
template <class C>
__device__ __forceinline__ int afrag_base(int rowi, int h, int m) {
    return (rowi * C::U16 + ((2 * m + h) ^ swz(rowi, C::SWB))) * 16;
}
// ... and the A-fragment of step t of the chunk living in ring slot `slot_off` (bytes); abase[m] = afrag_base(rowi, h, m)
template <class C>
__device__ __forceinline__ f32x4 afrag_read(const char* ring, const int (&abase)[C::SWB / 2], int slot_off, int t) {
    const int off = abase[t % (C::SWB / 2)] + (t / (C::SWB / 2)) * (C::SWB * 16);
    return *(const f32x4*)(ring + slot_off + off);
}

// ---- append protocol of the LDS candidate slots: reserve by popcount (ds_add_rtn on the slot's count), store with append_key, wait,
// then compact the slots full_slots names.  The reserve / wait statements themselves are each kernel's own (scan_topk.hip splits them
// around its cycle counters).
// one key of an append round, stored at wr_addr (advanced) in the lanes that pass.  No branch and no EXEC games (32 EXEC rewrites per
// tile stalled the MFMA stream for thousands of cycles): every lane stores, the non-passing ones into their private trash slot
__device__ __forceinline__ void append_key(bool pass, u32& wr_addr, u32 trash_addr, u64 key) {
    lds_store_b64_nofence(pass ? wr_addr : trash_addr, key);
    wr_addr += pass ? 8u : 0u;
}
// slots of this wave (bit jj = slot jj) that the A appends of the next round could overflow: to be compacted now
template <class C>
__device__ __forceinline__ u32 full_slots(const u32* cnt_w, int j) {
    const u32 c = cnt_w[j];
    const u64 bal = __ballot(c > (u32)(C::CAP - C::A));
    return (u32)bal | (u32)(bal >> 32);
}

// final: sort every slot of this wave, emit k keys per (part, query).  q_base = the wave's first query; nq_eff = queries that exist
// for this launch (<= nq, the stride of `partial`)
template <class C>
__device__ __forceinline__ void emit_slots(const u64* cand_w, const u32* cnt_w, u64* partial, int part, int q_base, int nq_eff, int nq,
                                           int k, int lane) {
    for (int jj = 0; jj < 32; ++jj) {
        const int qq = q_base + jj;
        if (qq >= nq_eff) break;
        const u32 n = cnt_w[jj];
        u64 key[C::NPL];
        u32 rank[C::NPL];
#pragma unroll
        for (int p = 0; p < C::NPL; ++p) {
            const u32 e = lane + 64 * p;
            key[p] = (e < n) ? cand_w[jj * C::CAP + e] : 0ull;
        }
        rank_keys<C::NPL>(key, n, rank);
        u64* dst = partial + ((size_t)part * nq + qq) * k;
#pragma unroll
        for (int p = 0; p < C::NPL; ++p) {
            const u32 e = lane + 64 * p;
            if (e < n) {
                if (rank[p] < (u32)k) dst[rank[p]] = key[p];
            } else if (e < (u32)k) {
                dst[e] = 0ull;   // fewer than k candidates: pad (e >= n are exactly the unfilled ranks)
            }
        }
    }
}

// launch Kernel with configuration C's dynamic LDS; the attribute is set once per instantiation
template <class C, auto Kernel, int BLOCK = 256, class L>
int launch_cfg(const L* p, hipStream_t s) {
    // function-local static: initialised exactly once, thread-safe (C++11)
    static const hipError_t attr_rc = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, C::LDS_BYTES);
    if (attr_rc != hipSuccess) return RMU_E_HIP;
    hipLaunchKernelGGL(Kernel, dim3(p->grid), dim3(BLOCK), C::LDS_BYTES, s, *p);
    return hipGetLastError() == hipSuccess ? RMU_OK : RMU_E_HIP;
}

// the padded row widths the scans are built for: f(integral_constant<int, dpad>)
template <class F>
int for_dpad(int dpad, F&& f) {
    switch (dpad) {
        case 384: return f(std::integral_constant<int, 384>{});
        case 768: return f(std::integral_constant<int, 768>{});
        case 192: return f(std::integral_constant<int, 192>{});
        default: return RMU_E_INVALID;
    }
}

}  // namespace

// rmu_common.h -- shared device/host helpers for librmu.so (gfx950 only).
#pragma once
#include <mutex>
#include <shared_mutex>
#include <vector>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;
typedef unsigned int u32;

// ---- candidate key: one u64 compares as (score desc, row asc) ---------------------------------
// hi 32 bits: order-preserving image of the fp32 score; lo 32 bits: ~row (smaller row = larger key).
// key 0 is the "no candidate" sentinel (smaller than every real key).
__host__ __device__ inline u32 rmu_f2ord(float f) {
    union { float f; u32 u; } c; c.f = f;
    return c.u ^ ((c.u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__host__ __device__ inline float rmu_ord2f(u32 o) {
    union { float f; u32 u; } c;
    c.u = o ^ ((o >> 31) ? 0x80000000u : 0xFFFFFFFFu);
    return c.f;
}
__host__ __device__ inline u64 rmu_make_key(float score, u32 row) {
    return ((u64)rmu_f2ord(score) << 32) | (u64)(u32)(~row);
}
__host__ __device__ inline float rmu_key_score(u64 k) { return rmu_ord2f((u32)(k >> 32)); }
__host__ __device__ inline u32 rmu_key_row(u64 k) { return ~(u32)k; }

// ---- wave-wide bitonic sort, descending, 64*NPL keys (lane holds elements lane + 64*p) ---------
template <int NPL>
__device__ __forceinline__ void rmu_bitonic_sort_desc(u64 (&key)[NPL], int lane) {
#pragma unroll
    for (int size = 2; size <= 64 * NPL; size <<= 1) {
#pragma unroll
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            if (stride >= 64) {
                const int ps = stride >> 6;
#pragma unroll
                for (int p = 0; p < NPL; ++p) {
                    if ((p & ps) == 0) {
                        const int p2 = p | ps;
                        const bool desc = (((lane + 64 * p) & size) == 0);
                        const u64 a = key[p], b = key[p2];
                        const u64 mx = a > b ? a : b, mn = a > b ? b : a;
                        key[p] = desc ? mx : mn;
                        key[p2] = desc ? mn : mx;
                    }
                }
            } else {
#pragma unroll
                for (int p = 0; p < NPL; ++p) {
                    const u64 other = __shfl_xor(key[p], stride);
                    const bool desc = (((lane + 64 * p) & size) == 0);
                    const bool lower = ((lane & stride) == 0);
                    const u64 mx = key[p] > other ? key[p] : other;
                    const u64 mn = key[p] > other ? other : key[p];
                    key[p] = (desc == lower) ? mx : mn;
                }
            }
        }
    }
}

// bitonic MERGE (input is a bitonic sequence of 64*NPL keys) -> sorted descending
template <int NPL>
__device__ __forceinline__ void rmu_bitonic_merge_desc(u64 (&key)[NPL], int lane) {
#pragma unroll
    for (int stride = 32 * NPL; stride > 0; stride >>= 1) {
        if (stride >= 64) {
            const int ps = stride >> 6;
#pragma unroll
            for (int p = 0; p < NPL; ++p) {
                if ((p & ps) == 0) {
                    const int p2 = p | ps;
                    const u64 a = key[p], b = key[p2];
                    key[p] = a > b ? a : b;
                    key[p2] = a > b ? b : a;
                }
            }
        } else {
#pragma unroll
            for (int p = 0; p < NPL; ++p) {
                const u64 other = __shfl_xor(key[p], stride);
                const bool lower = ((lane & stride) == 0);
                const u64 mx = key[p] > other ? key[p] : other;
                const u64 mn = key[p] > other ? other : key[p];
                key[p] = lower ? mx : mn;
            }
        }
    }
}

// Tuning / experiment switches (RMU_GEMM3, RMU_SCREEN_PACE, ...) are honoured ONLY when RMU_TUNING=1 is set as well: a stray
// RMU_* variable in a server's environment cannot change which kernels run.  Every switch is read once per process.  A process that
// sets RMU_* variables WITHOUT the master switch is told so once on stderr (they used to be honoured: silence would hide the change).
extern "C" char** environ;
inline const char* rmu_env(const char* name) {
    static const bool on = [] {
        const char* t = getenv("RMU_TUNING");
        const bool o = t != nullptr && atoi(t) == 1;
        if (!o && environ) {
            for (char** e = environ; *e; ++e)
                // (RMU_BENCH_* / RMU_REFERENCE_DIR belong to bench.py and the tests, not to the library)
                if (!strncmp(*e, "RMU_", 4) && strncmp(*e, "RMU_TUNING=", 11) && strncmp(*e, "RMU_SCREEN=", 11) && strncmp(*e, "RMU_GRAPH=", 10) &&
                    strncmp(*e, "RMU_BENCH_", 10) && strncmp(*e, "RMU_REFERENCE_DIR=", 18)) {
                    fprintf(stderr, "librmu: %.*s is set but ignored: tuning switches are honoured only with RMU_TUNING=1 (DESIGN.md 6.1)\n",
                            (int)(strchr(*e, '=') ? strchr(*e, '=') - *e : (long)strlen(*e)), *e);
                    break;
                }
        }
        return o;
    }();
    return on ? getenv(name) : nullptr;
}
// The two SAFETY kill switches deployments may rely on -- RMU_SCREEN=0 (no fp16 screening image: every search is the exact fp32 scan) and
// RMU_GRAPH=0 (rmu_bert_encode_host never captures a hipGraph) -- are honoured with or without the master switch: they only ever select
// the more conservative path.
inline const char* rmu_env_kill(const char* name) { return getenv(name); }

// ---- hipGraph captures in the same process (round 6; measured: tools/ubench/capture_probe.hip -> profiles/r06_capture_probe.txt) ----------
// The reference runs its LLM (PyTorch) on the same GPU and in the same process as this library (server/RAGHelper_local.py:42-105); a
// torch.cuda.graph capture there uses the GLOBAL capture mode.  On ROCm 7 a second thread whose capture-interaction mode is the default
// invalidates such a capture with nearly any synchronous call (hipMalloc, hipFree, hipStreamSynchronize, hipEventSynchronize,
// hipEventQuery, hipHostMalloc ...); with the thread's mode exchanged to RELAXED -- what PyTorch's own allocator does around
// cudaMalloc -- every one of them is harmless, EXCEPT hipDeviceSynchronize and the synchronous (pageable) hipMemcpy / hipMemset, which
// break a capture on another thread in every mode (and did break this library's own thread-local captures in round 5).  Hence:
//   1. every entry point runs under RMU_ENTRY(): the calling thread is in relaxed mode for the duration of the call;
//   2. the library never calls hipDeviceSynchronize, hipMemcpy or hipMemset: it waits for exactly the streams / events that used a
//      buffer (the index's reader events, a context's tail event) and copies with hipMemcpyAsync + hipStreamSynchronize.
struct RmuRelaxedCapture {
    hipStreamCaptureMode m = hipStreamCaptureModeRelaxed;
    RmuRelaxedCapture() { (void)hipThreadExchangeStreamCaptureMode(&m); }
    ~RmuRelaxedCapture() { (void)hipThreadExchangeStreamCaptureMode(&m); }
    RmuRelaxedCapture(const RmuRelaxedCapture&) = delete;
    RmuRelaxedCapture& operator=(const RmuRelaxedCapture&) = delete;
};
#define RMU_ENTRY() RmuRelaxedCapture rmu_relaxed_capture_
// This library's own captures (the host-path forwards of bert.hip, thread-local mode) are taken one at a time (round 5: two threads
// capturing at once failed 1 run in 4 on this runtime).
inline std::mutex& rmu_capture_mutex() {
    static std::mutex* mu = new std::mutex;      // (never destroyed: thread-local workspaces are released while the process winds down)
    return *mu;
}
// hipFree waits for the device by itself; in relaxed mode it leaves captures of other threads alone (probe above)
inline hipError_t rmu_free(void* p) {
    RMU_ENTRY();
    return hipFree(p);
}

// ---- launch descriptors shared between rmu_api.hip and the kernel translation units -------------
// Device-side launch predicate.  The screening path decides per query ON THE DEVICE whether the exact scan has to re-run
// it; the re-run launches are enqueued unconditionally and every workgroup of a launch whose predicate is false returns
// at once, so a search never needs a host round trip (and honours a caller-supplied stream).
//   p == null: always run.  Otherwise c = *p (number of flagged queries): run iff lo <= c <= hi; clamp != 0: only the first
//   min(nq, c) queries of the launch exist.
struct RmuCond {
    const int* p;
    int lo, hi, clamp;
};

struct ScanLaunch {
    const float* x;        // [n_rows, dpad] fp32 row-major, HBM resident
    int64_t n_rows;
    int64_t row0;          // first row of the scanned range: screening scan rows [row0, row0 + n_rows) of the image `x`; exact scan: `x`
                           // already points at row row0 and row0 is only added to the row ids of the keys
    int dpad;              // row stride in floats (192 / 384 / 768; scan_wide_kernel: a multiple of 32)
    const float* q;        // [nq, dpad] fp32 device (padded like the rows)
    int nq;
    int k;
    u64* partial;          // [parts, nq, k] keys
    int share_thr;         // bit 0 = read the shared thresholds (0: publish only; debugging aid); bit 1 = no filter (timing ablation); bit 2 (screening scan) =
                           // emit slots of <= k entries unsorted (the launch's merge must be told: rmu_merge_to_keys_launch(..., unsorted = 1));
                           // bit 3 (screening scan, spill launches) = every wave re-reads and refreshes its thresholds at every pair of tiles
                           // (RMU_OPT_SCREEN_REFRESH = 1; 0: only the waves that can use them -- scan_screen.hip "Refresh")
    u32* gthr;             // [nq] shared per-query threshold (order-preserving u32 image, 0 = none), zeroed per launch
    int parts;             // filled by the planner
    u64* dbg;              // optional debug counters (nullptr in production): [0] slow tiles, [1] compactions, [2] appends, [3] tiles ... [16] pair prologue cycles
    // filled by rmu_scan_plan
    int wq, kv, s_chunks, nqt, tiles_per_chunk, grid, lds_bytes;
    int qg;                // screening scan only: 32-query groups per wave, always 1 (rmu_screen_plan)
    int nt;                // 1 = stream the corpus with non-temporal loads (every byte is read by exactly one workgroup)
    RmuCond cond;          // exact scan only: device-side launch predicate (zero-initialised = always)
    // screening scan only: sibling pacing (scan_screen.hip).  prog = [s_chunks][4] progress words of the query-tile workgroups
    // of each row chunk (zeroed per launch; nullptr = off), pace = how many tiles a workgroup may run ahead of its slowest sibling
    u32* prog;
    int pace;
    // screening scan only (scan_screen.hip): candidate slots in global memory, [parts][nq][CAP] keys (RMU_KS_CAP, or RMU_KS_CAP_DEEP for
    // deep K').  Needs no initialisation (the slot counts live in registers); contents are dead once the launch has written its partials
    u64* gcand;
    // screening scan of an RMU_METRIC_L2SQ index: -2048 |x|^2 per image row (indexed like the image: row0 is added); nullptr = inner product
    const float* nrm;
    // exact scan only: 1 = scan_wide_kernel (scan_wide.hip: queries streamed through the ring, any dpad that is a multiple of 32 up to 3072).  Set by
    // rmu_scan_plan for dpad > 768, or by the caller in front of it (RMU_OPT_WIDE_SCAN) for a width scan_topk_kernel would take
    int wide;
    // screening scan only, seeded launches of the 8-wave kernels (scan_screen.hip, "Spill path"): a lane whose running maximum beats its query
    // group's threshold writes its 8 accumulators of that group + (tile, lane, group) as one RMU_SPILL_REC-byte record into the list of its
    // (row chunk, query tile, wave); rmu_sift_launch files the records.  spill = nullptr: off (every passing tile takes slow_path)
    char* spill;           // [s_chunks * nqt * 8][spill_cap] records
    u32* spill_cnt;        // [s_chunks * nqt * 8] records written; bit 31 = the wave ran out of room and went on through slow_path (its slots are emitted)
    int spill_cap;         // records per list
};
#define RMU_SPILL_REC 48  /* 8 fp32 accumulators (element 4 t + c = tile row 16 t + 4 (lane >> 4) + c) + {tile of the chunk, lane | group << 8, 0, 0} */
#define RMU_SPILL_FELL 0x80000000u
#define RMU_KS_CAP 48    /* K' <= 40 kept candidates + 8 free slots between compactions (one key per lane in the rank: <= 64) */
#define RMU_KS_CAP_DEEP 128   /* (round 6) 32 < k <= 104: K' <= 120 kept candidates + 8 free slots, two keys per lane in the rank */

// Row chunks of a scan launch of nqt query tiles over tiles_total row tiles (every planner's: rmu_scan_plan, rmu_subset_plan,
// rmu_screen_plan): a multiple of 8 (XCD-aware block map) that makes grid = s_chunks * nqt fill 256 CUs evenly
inline void rmu_plan_chunks(int nqt, int64_t tiles_total, int* s_chunks, int* tiles_per_chunk) {
    int best_s = 8;
    double best_eff = -1.0;
    for (int s = 8; s <= 256; s += 8) {
        const int64_t total = (int64_t)s * nqt;
        const double eff = (double)total / (double)(((total + 255) / 256) * 256);
        if (eff > best_eff + 1e-9) { best_eff = eff; best_s = s; }
        if (total >= 256 && eff > 0.999) break;
    }
    int s = best_s;
    if (tiles_total < s) s = tiles_total > 0 ? (int)tiles_total : 1;
    *tiles_per_chunk = (int)((tiles_total + s - 1) / s);
    if (*tiles_per_chunk < 1) *tiles_per_chunk = 1;
    // drop empty trailing chunks (keeps the multiple-of-8 property only when nothing is dropped)
    const int64_t used = (tiles_total + *tiles_per_chunk - 1) / *tiles_per_chunk;
    if (used > 0 && used < s) s = (int)used;
    *s_chunks = s;
}

// ---- the one-call hybrid (rrf_fuse.hip) borrows the first halves of the members' searches: everything enqueued on ONE stream, results left on
// the device, the member's shared lock handed back held (the caller releases it once it has drained the stream) --------------------------------
struct rmu_index;
struct rmu_bm25;
int rmu_thread_stream_(hipStream_t user, hipStream_t* s);         // rmu_api.hip: the stream a call of this thread runs on (user, or the thread's own)
void rmu_thread_finished_(hipStream_t s, bool drained);           // rmu_api.hip: end of a call that used the thread's workspaces on s
// *d_rows: [nq, k] int64 row ids in pick order (-1 = none); expect_rows >= 0: RMU_E_INVALID ("out of step") unless the index holds that many rows
int rmu_index_search_mmr_enqueue_(rmu_index* idx, const float* q, bool q_dev, int64_t nq, int fetch_k, int k, double lambda_mult, int64_t expect_rows,
                                  hipStream_t s, const char* who, std::shared_lock<std::shared_mutex>& lk, const int64_t** d_rows);
// *d_docs: [nq, k] int64 document ids, best first (-1 = none); *empty: no live document, nothing enqueued; expect_docs as expect_rows
int rmu_bm25_search_enqueue_(rmu_bm25* h, const char* query_blob, int64_t bytes, int64_t nq, int k, int64_t expect_docs, hipStream_t stream,
                             std::shared_lock<std::shared_mutex>& lk, const int64_t** d_docs, bool* empty);

int rmu_device_ordinal();                                // the device rmu_init chose, -1 before it (rmu_api.hip): per-thread contexts of other units follow it
int rmu_scan_plan(ScanLaunch* p);                        // chooses geometry; returns 0 or RMU_E_INVALID
int rmu_scan_launch(const ScanLaunch* p, hipStream_t s); // launches the fused scan
int rmu_wide_plan(ScanLaunch* p);                        // the same pair for scan_wide_kernel; rmu_scan_plan / rmu_scan_launch route to it
int rmu_wide_launch(const ScanLaunch* p, hipStream_t s);
int rmu_merge_final_launch(const u64* partial, int parts, int64_t nq, int k, int64_t row_base, int l2_out, const float* qnorm2,
                           float* out_scores, int64_t* out_rows, const int64_t* scatter /* or null */, const RmuCond* cond /* or null */,
                           hipStream_t s);
int rmu_merge_to_keys_launch(const u64* partial, int parts, int64_t nq, int k, u64* out_keys, u32* seed_thr /* or null */,
                             hipStream_t s, int unsorted = 0 /* the lists are compact but not sorted (ScanLaunch::share_thr bit 2) */);
// the same merge; seed_thr also receives the lower edge of the sufficiency band of the caller's k = band_k < k (band_eps: EPS(q) per query, or null)
int rmu_merge_to_keys_band_launch(const u64* partial, int parts, int64_t nq, int k, u64* out_keys, u32* seed_thr, hipStream_t s, int unsorted,
                                  int band_k, const float* band_eps);
// the merge of a seeded launch that spilled (S.spill != nullptr; topk_merge.hip: sift_kernel): the running top-k `running` [nq, k] + the
// launch's spill records above gthr[q] + the part lists S.partial of the waves that fell back -> out_keys [nq, k]; seeds as the band merge does
int rmu_sift_launch(const ScanLaunch* S, const u64* running, int64_t nq, int k, u64* out_keys, u32* seed_thr, hipStream_t s, int band_k,
                    const float* band_eps);
// fp16 screening path (scan_screen.hip)
#define RMU_IMG_ROW_BYTES 768                        /* fp16(64 x) image of a 384-d row */
int rmu_split_launch(const float* src, void* dst, int64_t n_rows, hipStream_t s, int stride = 384,
                     float scale = 64.0f, u32* zero_a = nullptr, int n_zero_a = 0, u32* zero_b = nullptr, int n_zero_b = 0,
                     float* eps_out = nullptr /* [n_rows]: EPS(q) of each row taken as a query (l2: rows are (2q, 1)) */, float xnorm_max = 0.f,
                     float dx_max = 0.f, int l2 = 0);                                             // fp32 [n, 384 of stride] -> fp16(scale x) image
int rmu_screen_launch(const ScanLaunch* p, hipStream_t s);                             // x/q = split images, k = K'
int rmu_screen_plan(ScanLaunch* p);                      // geometry of one screening launch (k = K' <= 32)
int rmu_img_err_launch(const float* x, int64_t n_rows, float* err2, hipStream_t s, int stride = 384);   // |x - image|^2 per row
// stride = floats between rows of x AND of q; qn2_l2 (RMU_METRIC_L2SQ: |q|^2 per query; x and q in the L2 index's augmented form) or null
int rmu_rescore_launch(const u64* cand, int kp, const float* x, const float* q, int64_t nq, int k, float xnorm_max, float dx_max,
                       int64_t row_base, float* out_s, int64_t* out_r, int* flagged /* [0] = count */, int64_t* flagged_list,
                       float* eps_out /* or null */, hipStream_t s, int stride = 384, const float* qn2_l2 = nullptr);
// shard lists [parts][nq, k]: part p's scores start at scores + p * stride_s (floats), rows at rows + p * stride_r (int64);
// smaller_better: distances (RMU_METRIC_L2SQ) instead of similarities
int rmu_merge_lists_launch(const float* scores, const int64_t* rows, int parts, int64_t stride_s, int64_t stride_r, int64_t nq, int k,
                           int smaller_better, float* out_scores, int64_t* out_rows, hipStream_t s);

// gathered exact scan of rmu_index_search_subset (scan_subset.hip): the rows named by one ascending list, keys carry list positions
struct SubsetLaunch {
    const float* x;        // [n_rows, dpad] fp32 row-major: the index's matrix
    int64_t n_rows;        // rows of the index: an id outside [0, n_rows) is absent
    int dpad;
    const u32* ids;        // [rmu_subset_ids_len(n_sub)] narrowed list (rmu_subset_narrow_launch), 0xFFFFFFFF = absent / padding
    int64_t n_sub;
    const float* q;        // [nq, dpad] fp32 device, prepared like rmu_index_search's
    int nq;
    int k;
    u64* partial;          // [parts, nq, k] keys (score, list position)
    u32* gthr;             // [nq padded to 128] shared thresholds: published, never read
    // filled by rmu_subset_plan
    int wq, kv, s_chunks, nqt, tiles_per_chunk, grid, parts, lds_bytes;
};
int64_t rmu_subset_ids_len(int64_t n_sub);               // u32 entries of the narrowed list (whole tiles + one tile of padding)
int rmu_subset_plan(SubsetLaunch* p);
int rmu_subset_launch(const SubsetLaunch* p, hipStream_t s);
int rmu_subset_narrow_launch(const int64_t* rows, int64_t n_sub, int64_t n_rows, u32* ids, hipStream_t s);
int rmu_subset_map_launch(int64_t* out_rows, const u32* ids, int64_t total, int64_t row_base, hipStream_t s);   // position -> row id + row_base

// ---- the grouped form (rmu_index_search_groups): one list per group of adjacent queries, every group in one launch per geometry class ----
// what ONE workgroup of scan_groups_kernel does (scan_subset.hip: subset_scan's arguments)
struct GroupDesc {
    u32 ids_off;           // where its list starts in the narrowed ids (a multiple of 128)
    u32 t0, ntiles;        // its tiles of that list (tiles of its class: 128 rows with wq = 1, 32 with wq = 4); ntiles = 0: nothing to scan
    u32 q_first, q_end;    // its 32 * wq queries start at q_first (ANY index); those below q_end, the end of the group, exist
    u32 part0;             // its first part of `partial` (list chunk * (4 / wq))
    u32 pad[2];
};
// one list that some query uses: rows[src .. src + len) of the caller's array -> ids[ids_off .. ids_off + rmu_subset_ids_len(len))
struct GroupList { int64_t src; u32 len, ids_off; };
struct GroupsLaunch {
    const float* x; int64_t n_rows; int dpad;
    const u32* ids;        // every used list narrowed, each padded as rmu_subset_ids_len pads one, end to end
    const float* q; int nq; int k;
    u64* partial;          // [parts, nq, k], ZEROED by the caller: a group with fewer parts leaves empty lists
    u32* gthr;             // [nq + 128]: published, never read (a tile of queries may start anywhere below nq)
    const GroupDesc* tab;  // [grid] device
    int wq, kv, grid, lds_bytes;
};
// the host's plan of a call: the work tables of the two geometry classes (0: wq = 1, 1: wq = 4), the used lists, each query's ids_off
struct GroupsPlan {
    std::vector<GroupDesc> tab[2];
    std::vector<GroupList> lists;
    std::vector<u32> q_off;
    int64_t ids_total = 0;     // u32 entries of the narrowed ids
    int parts = 1;             // P of the merge: the largest part count of any group
    int lds_bytes[2] = {0, 0};
};
int rmu_groups_plan(int dpad, int k, int nq, const int64_t* list_ptr, const int32_t* q_list, GroupsPlan* out);
int rmu_groups_launch(const GroupsLaunch* p, hipStream_t s);
int rmu_groups_narrow_launch(const int64_t* rows, const GroupList* lists, int n_lists, int64_t n_rows, u32* ids, int64_t ids_total, hipStream_t s);
// position in the query's own list -> row id + row_base; q_off [nq]: where that list starts in ids
int rmu_groups_map_launch(int64_t* out_rows, const u32* ids, const u32* q_off, int64_t total, int k, int64_t row_base, hipStream_t s);

// ---- grouped top-k (rmu_index_search_distinct; scan_distinct.hip): the best row of each of the k best groups, contiguous rows ----------
struct DistinctLaunch {
    const float* x;        // [n_rows, dpad] fp32 row-major: the index's matrix
    int64_t n_rows;
    int dpad;
    const int32_t* codes;  // [n_rows] device: the group of every row (one field of the columns' image)
    const float* q;        // [nq, dpad] fp32 device, prepared like rmu_index_search's
    int nq;
    int k;                 // <= RMU_MAX_K_DISTINCT
    u64* partial;          // [parts, nq, k] keys: every part list sorted, distinct inside, zeros last
    // filled by rmu_distinct_plan
    int wq, s_chunks, nqt, tiles_per_chunk, grid, parts, lds_bytes;
};
int rmu_distinct_plan(DistinctLaunch* p);
int rmu_distinct_launch(const DistinctLaunch* p, hipStream_t s);
// part lists [parts <= 1024, nq, k] -> out_keys [nq, k]: one distinct list per query, sorted, zero-padded (rmu_merge_final_launch with parts = 1 finishes it)
int rmu_distinct_fold_launch(const u64* partial, int parts, int64_t nq, int k, const int32_t* codes, u64* out_keys, hipStream_t s);
// rmu_api.hip, behind rmu_index_search_distinct (columns.hip, which holds the columns' shared lock and has settled their image): the scan, the
// fold and rmu_index_search's finishing; RMU_E_INVALID ("out of step") unless the index holds expect_rows rows; always drains its stream
int rmu_index_search_distinct_on_(rmu_index* idx, const int32_t* codes_dev, int64_t expect_rows, const float* q, int64_t nq, int k, unsigned flags,
                                  int64_t row_base, float* out_scores, int64_t* out_rows, hipStream_t user_stream);

// row moves of rmu_index_compact (rmu_compact.hip), one array of the index at a time: rows of row_bytes (a multiple of 256, or 4 for the
// L2 norms); new row j in [first, n_live) comes from old row src_rows[j - first] (device list, strictly increasing, src_rows[i] >= first + i);
// rows [0, first) stay where they are.
//   alloc_rows > 0: out of place -- a new allocation of alloc_rows rows (capacity + slack) receives the prefix and the gathered rows, its
//     rows [n_live, alloc_rows) are set to the byte `fill`, the stream is drained and the old allocation freed (*base = the new one).  A
//     failed allocation returns hipErrorOutOfMemory with nothing moved.
//   alloc_rows == 0: in place, chunk by chunk through `staging`, then rows [n_live, n_old) are set to `fill`; enqueues only.
hipError_t rmu_compact_array(void** base, int64_t row_bytes, int fill, int64_t n_old, int64_t n_live, int64_t first, const u32* src_rows,
                             int64_t alloc_rows, void* staging, size_t staging_bytes, hipStream_t s);

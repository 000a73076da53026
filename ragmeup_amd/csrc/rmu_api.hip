// rmu_api.hip -- C-ABI of librmu.so (see include/rmu.h): HBM-resident flat index + search orchestration.
//
// Reference call sites served (server/ = /root/reference/server):
//   rmu_index_create      RAGHelper.py:385-404   (Milvus.from_documents([],...) / PGVector(...))
//   rmu_index_add         RAGHelper.py:431, 525  (db.add_documents(documents, ids=ids))
//   rmu_index_search      RAGHelper.py:497-499   (dense retriever -> FLAT similarity search)
//   rmu_index_get_rows    RAGHelper.py:497-499   (search_type="mmr": re-fetch the fetch_k vectors)
//   rmu_index_search_subset RAGHelper.py:497-499 (the same retriever with search_kwargs: Milvus col.search(expr=...) / PGVector filter=)
//   rmu_index_remove_rows server.py:373-377      (collection.delete('source == ...'))
//   rmu_index_compact     server.py:353-385 + RAGHelper.py:518-538 (delete / re-upload cycle; row moves in rmu_compact.hip)
//   rmu_topk_merge        no counterpart (8-GPU shard merge)
//
// Data layout in HBM: one row-major [capacity, dpad] fp32 matrix, dpad = dim rounded up to 192/384/768, above 768 to the next multiple of 64
// (zero padded), base 256-B aligned so every 1536-B row of the 384-d flagship is 12 full 128-B lines.
// Tombstoned rows are NaN-poisoned in place: every score against them is NaN and fails the scan's
// `score > threshold` compare, so deletion costs nothing in the hot loop.
#include <mutex>
#include <chrono>
#include <shared_mutex>
#include <string>
#include <vector>
#include <cmath>
#include <cstdio>
#include <algorithm>
#include <cstring>
#include <cstdlib>

#include "rmu_common.h"
#include "rmu_host.h"
#include "../../include/rmu.h"
#include "rmu_internal.h"      // rmu_index_search_mmr_dev_: the prototype bert.hip calls it by

// ------------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------------
static thread_local std::string g_err;
extern "C" const char* rmu_last_error(void) { return g_err.c_str(); }
extern "C" void rmu_set_error_(const char* msg) { g_err = msg ? msg : ""; }   // behind rmu_fail (rmu_host.h)
extern "C" const char* rmu_version(void) { return "librmu 0.1 gfx950"; }

static int g_device = -1;
extern "C" int rmu_init(int device_ordinal) {
    RMU_ENTRY();
    int n = 0;
    RMU_HIP_TRY(hipGetDeviceCount(&n));
    if (device_ordinal < 0 || device_ordinal >= n) return rmu_fail(RMU_E_INVALID, "rmu_init: no such device");
    RMU_HIP_TRY(hipSetDevice(device_ordinal));
    g_device = device_ordinal;
    return RMU_OK;
}
int rmu_device_ordinal() { return g_device; }

// ------------------------------------------------------------------------------------------------
// per-thread context: stream, events, grow-only workspace
// ------------------------------------------------------------------------------------------------
// Set once the process starts tearing the HIP runtime down (static destructors / atexit): thread-local destructors
// that run after that point must not call into HIP any more (rmu_runtime_down, rmu_host.h: every unit's contexts ask here).
static bool g_runtime_down = false;
namespace { struct RuntimeGuard { ~RuntimeGuard() { g_runtime_down = true; } } g_runtime_guard; }
bool rmu_runtime_down() { return g_runtime_down; }

struct Tls {
    hipStream_t stream = nullptr;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    RmuDevBuf q, partial, out_s, out_r, in_s, in_r, qn, gthr, qsplit, ckeys, flag, nrm, fbq, fb_i, mm_q, mm_s, mm_r, mm_p, gcand, sub_ids, sub_rows, gtab, eps, spill, spill_cnt;
    std::vector<hipEvent_t> lev;   // per-launch events of the screening ladder
    int ensure_events(int n) {
        while ((int)lev.size() < n) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return RMU_E_HIP;
            lev.push_back(e);
        }
        return RMU_OK;
    }
    int* hflag = nullptr;          // pinned landing word of the screening path's re-run count
    int* hflag_dev = nullptr;      // ... as the device sees it (written by k_gather_flagged)
    RmuPinBuf hpin{4096};          // pinned landing buffer of search_mmr_on's results (rows | scores in ONE device-to-host copy)
    int ensure_hflag() {
        if (hflag) return RMU_OK;
        if (hipHostMalloc((void**)&hflag, sizeof(int)) != hipSuccess) { hflag = nullptr; (void)hipGetLastError(); return RMU_E_OOM; }
        *hflag = 0;
        if (hipHostGetDevicePointer((void**)&hflag_dev, hflag, 0) != hipSuccess) { (void)hipGetLastError(); hflag_dev = hflag; }   // (unified addressing: the same pointer)
        return RMU_OK;
    }
    bool timing = false;
    float scan_ms = -1.f, search_ms = -1.f;
    float fold_ms = -1.f;          // rmu_index_search_distinct under rmu_set_timing: k_distinct_fold's time, and the part lists it folded
    int fold_parts = 0;
    int grid = 0, block = 0, lds = 0, passes = 0, screened = 0;
    // what rmu_last_scan_geometry reports: the geometry of the last scan enqueued, the launches of the whole call
    template <class Launch>          // (ScanLaunch, SubsetLaunch)
    void note_geometry(const Launch& L, int launches) { grid = L.grid; block = 256; lds = L.lds_bytes; passes += launches; }
    int device = -1;
    // A search / merge given a caller stream and device buffers returns with its kernels still in flight -- on workspaces
    // (q, qsplit, partial, gthr, ckeys, flag, fbq, fb_i) that belong to this thread, not to that stream.  `pend_ev` marks the end
    // of the last such call: the next user of the workspaces on ANY OTHER stream is ordered behind it (same stream: stream
    // order already does that), so a second call can neither memset thresholds nor overwrite partials under running kernels.
    hipEvent_t pend_ev = nullptr;
    hipStream_t pend_stream = nullptr;
    bool pending = false;
    // `user`: the stream the caller's work will be enqueued on (nullptr = this thread's internal stream)
    int ensure_stream(hipStream_t user = nullptr) {
        rmu_follow_device(device);
        if (!stream) {
            if (hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) return RMU_E_HIP;
            for (auto& e : ev)
                if (hipEventCreate(&e) != hipSuccess) return RMU_E_HIP;
            if (hipEventCreateWithFlags(&pend_ev, hipEventDisableTiming) != hipSuccess) return RMU_E_HIP;
        }
        hipStream_t s = user ? user : stream;
        if (pending && s != pend_stream && hipStreamWaitEvent(s, pend_ev, 0) != hipSuccess) return RMU_E_HIP;
        return RMU_OK;
    }
    // end of a call that used the workspaces on stream s: either it synchronised s (everything pending was ordered before
    // its own work, so nothing is in flight any more) or it leaves work in flight there
    void finished(hipStream_t s, bool drained) {
        if (drained) { pending = false; return; }
        if (hipEventRecord(pend_ev, s) == hipSuccess) { pend_stream = s; pending = true; }
        else { (void)hipStreamSynchronize(s); pending = false; }
    }
    // A server that spawns a thread per request (Flask's threaded dev server, server/server.py:394) creates one of
    // these per request: everything it owns goes back when the thread exits.  Only what has an order is done here -- the work in flight
    // ends first; the workspaces free themselves (~RmuDevBuf, ~RmuPinBuf) once this body has run, i.e. behind the drained stream.
    ~Tls() {
        if (g_runtime_down) return;
        RMU_ENTRY();
        if (pending) (void)hipEventSynchronize(pend_ev);
        if (pend_ev) (void)hipEventDestroy(pend_ev);
        if (stream) (void)hipStreamSynchronize(stream);
        for (auto& e : ev)
            if (e) (void)hipEventDestroy(e);
        for (auto& e : lev) (void)hipEventDestroy(e);
        if (hflag) (void)hipHostFree(hflag);
        if (stream) (void)hipStreamDestroy(stream);
    }
};
static thread_local Tls g_tls;

extern "C" int rmu_last_screened(void) { return g_tls.screened; }
extern "C" int rmu_set_timing(int on) { g_tls.timing = on != 0; return RMU_OK; }
extern "C" float rmu_last_scan_ms(void) { return g_tls.scan_ms; }
extern "C" float rmu_last_search_ms(void) { return g_tls.search_ms; }
extern "C" int rmu_last_scan_geometry(int* grid, int* block, int* lds_bytes, int* passes) {
    if (grid) *grid = g_tls.grid;
    if (block) *block = g_tls.block;
    if (lds_bytes) *lds_bytes = g_tls.lds;
    if (passes) *passes = g_tls.passes;
    return RMU_OK;
}

// ------------------------------------------------------------------------------------------------
// small kernels
// ------------------------------------------------------------------------------------------------
__global__ void k_poison_rows(float* x, int dpad, const int64_t* rows, int64_t n) {
    const int64_t r = blockIdx.x;
    if (r >= n) return;
    float* row = x + rows[r] * (int64_t)dpad;
    for (int c = threadIdx.x; c < dpad; c += blockDim.x) row[c] = __builtin_nanf("");
}

// one wave per row: x <- x / max(|x|, 1e-12) (rows of `dpad` floats, pad columns are zero);
// optionally also writes |x|^2 (before normalisation) to norm2[r]
__global__ void k_row_norm(float* x, int dpad, int64_t n, int normalise, float* norm2) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= n) return;
    float* row = x + r * (int64_t)dpad;
    float s = 0.f;
    for (int c = lane; c < dpad; c += 64) s = fmaf(row[c], row[c], s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (norm2 && lane == 0) norm2[r] = s;
    if (normalise) {
        const float inv = 1.0f / fmaxf(sqrtf(s), 1e-12f);
        for (int c = lane; c < dpad; c += 64) row[c] *= inv;
    }
}

// RMU_METRIC_L2SQ: the scan ranks by inner product, and argmin |q - x|^2 = argmax (2 q.x - |x|^2).  Rows carry -|x|^2 in
// the first pad column (column `dim`; the L2 index pads dim + 1), queries are stored as (2q, 1): the scan's inner product
// is then 2 q.x - |x|^2 and the merge reports |q|^2 minus it.  One wave per row.
__global__ void k_l2_aug_rows(float* x, int dpad, int dim, int64_t n) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= n) return;
    float* row = x + r * (int64_t)dpad;
    float s = 0.f;
    for (int c = lane; c < dim; c += 64) s = fmaf(row[c], row[c], s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) row[dim] = -s;
}
// queries (already copied into the dpad-wide buffer): qn2[r] = |q|^2, q <- 2q, column dim <- 1
__global__ void k_l2_aug_queries(float* q, int dpad, int dim, int64_t n, float* qn2) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= n) return;
    float* row = q + r * (int64_t)dpad;
    float s = 0.f;
    for (int c = lane; c < dim; c += 64) { const float v = row[c]; s = fmaf(v, v, s); row[c] = 2.0f * v; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) { qn2[r] = s; row[dim] = 1.0f; }
}

// L2 index with a screening image: nrm[r] = -2048 |x_r|^2 (the accumulator start of scan_screen_lean3_kernel's L2 form: the stored -|x|^2
// column times 2^11, exact) and norm2[r] = |x_r|^2 for the |x|max statistic
__global__ void k_l2_nrm(const float* __restrict__ x, int dpad, int dim, int64_t n, float* __restrict__ nrm, float* __restrict__ norm2) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const float v = x[r * (int64_t)dpad + dim];
    if (nrm) nrm[r] = 2048.0f * v;
    norm2[r] = -v;
}

// max over rows of |x|^2 (non-negative floats order like their bit patterns)
__global__ void k_max_norm2(const float* __restrict__ norm2, int64_t n, unsigned* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    float v = i < n ? norm2[i] : 0.f;
    if (!(v == v)) v = 0.f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0) atomicMax(out, __float_as_uint(v));
}

__global__ void k_gather_rows(const float* x, int dpad, int dim, const int64_t* rows, int64_t n, float* out) {
    const int64_t r = blockIdx.x;
    if (r >= n) return;
    const float* row = x + rows[r] * (int64_t)dpad;
    for (int c = threadIdx.x; c < dim; c += blockDim.x) out[r * dim + c] = row[c];
}

// the queries the screening path flagged (list `pos`, count *count) -> a dense [count, dpad] block for the exact re-run
// (round 6, second session) ... and the two other things the conditional re-runs need, in the same launch (every dependent stream operation
// costs ~4.5 us of kernel boundary behind a search): the shared thresholds of the re-run launches zeroed (was a memset), the count landed in
// pinned host memory for rmu_last_screened (was a device-to-host copy at the end).  gather_n = 0: a batch of <= 32 queries re-runs as a whole.
__global__ void k_gather_flagged(const float* __restrict__ q, int dpad, const int64_t* __restrict__ pos, const int* __restrict__ count,
                                 float* __restrict__ out, int gather_n, u32* __restrict__ zero_words, int n_zero, int* __restrict__ host_count) {
    const int64_t r = blockIdx.x;
    const int cnt = *count;
    if (r == 0) {
        for (int i = threadIdx.x; i < n_zero; i += blockDim.x) zero_words[i] = 0u;
        if (threadIdx.x == 0 && host_count) *host_count = cnt;
    }
    if (r >= gather_n || r >= cnt) return;
    const float* row = q + pos[r] * (int64_t)dpad;
    for (int c = threadIdx.x; c < dpad; c += blockDim.x) out[r * dpad + c] = row[c];
}

// Batched greedy MMR (langchain_core `maximal_marginal_relevance`, the reference retriever's search_type="mmr",
// server/RAGHelper.py:497-499): one wave per query, lane i = candidate i (fetch_k <= 64), fp64 like the numpy original.
//   first pick = argmax_i cos(q, x_i); then repeatedly argmax_i  lambda*cos(q, x_i) - (1-lambda)*max_{s picked} cos(x_i, x_s),
//   strict '>' so the lowest index wins ties; cos = dot / (|a||b|), NaN/inf -> 0.
// rows: [nq, fetch_k] index-local row ids (-1 = absent, as rmu_index_search pads them; so is an id >= n_rows and a REMOVED row, whose
// norm is NaN: never picked, not counted); out_pos: [nq, k] positions in the candidate list, -1 past the number of candidates.
__global__ __launch_bounds__(256) void k_mmr(const float* __restrict__ x, int dpad, int dim, int64_t n_rows,
                                             const float* __restrict__ q, const int64_t* __restrict__ rows, int64_t nq,
                                             int fetch_k, int k, double lambda, int* __restrict__ out_pos) {
    const int lane = threadIdx.x & 63;
    const int64_t qi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= nq) return;
    const int64_t row = lane < fetch_k ? rows[qi * fetch_k + lane] : -1;
    const bool in_index = row >= 0 && row < n_rows;
    const float* xr = x + (in_index ? row : 0) * (int64_t)dpad;
    const float* qv = q + qi * dim;
    double dq = 0.0, nx = 0.0, nqq = 0.0;
    for (int c = 0; c < dim; ++c) {
        const double a = (double)xr[c], b = (double)qv[c];
        dq = fma(a, b, dq);
        nx = fma(a, a, nx);
        nqq = fma(b, b, nqq);
    }
    nx = sqrt(nx); nqq = sqrt(nqq);
    const bool valid = in_index && nx == nx;          // a removed row is NaN-poisoned: its norm is NaN and the candidate is ABSENT, like a -1
    double sim_q = dq / (nx * nqq);
    if (!(sim_q == sim_q) || isinf(sim_q)) sim_q = 0.0;
    const int n_valid = __builtin_popcountll(__ballot(valid));
    const int want = k < n_valid ? k : n_valid;
    // wave argmax with the lowest lane on ties
    auto argmax = [&](double v, bool ok) -> int {
        double m = ok ? v : -INFINITY;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o));
        const unsigned long long eq = __ballot(ok && v == m);
        return eq ? __builtin_ctzll(eq) : -1;
    };
    bool picked = false;
    double red = -INFINITY;          // max cosine to the picked set
    int sel = argmax(sim_q, valid);
    for (int t = 0; t < want && sel >= 0; ++t) {
        if (lane == 0) out_pos[qi * k + t] = sel;
        if (lane == sel) picked = true;
        if (t + 1 == want) break;
        // cosine of every candidate to the newly picked one
        const int64_t srow = __shfl(row, sel);
        const double ns = __shfl(nx, sel);
        const float* xs = x + srow * (int64_t)dpad;
        double d = 0.0;
        for (int c = 0; c < dim; ++c) d = fma((double)xr[c], (double)xs[c], d);
        double cs = d / (nx * ns);
        if (!(cs == cs) || isinf(cs)) cs = 0.0;
        red = fmax(red, cs);
        sel = argmax(lambda * sim_q - (1.0 - lambda) * red, valid && !picked);
    }
    for (int t = want + lane; t < k; t += 64) out_pos[qi * k + t] = -1;
}

// The same selection for ONE query per workgroup with the candidates staged in LDS and their GRAM MATRIX computed up front by all 256
// threads (round 4).  k_mmr's lane walks its own row in global memory one float at a time (a dependent load per fp64 fma: 0.32 ms for
// the reference's per-request call, 20 candidates, 10 picks); round 3 staged the rows in LDS and ran the unchanged chain on wave 0 --
// still one 384-step fp64 chain per pick and lane, 58 us.  Every cosine the greedy loop can ask for is an entry of G = X X^T, so:
//   1. all threads copy the <= 64 rows (coalesced) into LDS rows of dim + 1 floats (odd stride: conflict-free column walks) and q;
//   2. one task per thread: G[i][j] for i <= j, q . x_i, q . q -- fp64 fma over the dims, FOUR interleaved partial chains
//      ((s0 + s1) + (s2 + s3): the chain length, not the issue rate, bounded the old kernel); 231 tasks for 20 candidates = one round;
//   3. wave 0 runs the greedy loop on look-ups: cos(x_i, x_sel) = G[i][sel] / (|x_i| |x_sel|).
// Same rule and tie order as k_mmr (langchain's); the fp64 sums differ from k_mmr's in the last bits only (summation order).
// dim <= 384: 98.6 KiB of rows + 32.5 KiB of G.
__global__ __launch_bounds__(256) void k_mmr_lds(const float* __restrict__ x, int dpad, int dim, int64_t n_rows,
                                                 const float* __restrict__ q, const int64_t* __restrict__ rows, int64_t nq,
                                                 int fetch_k, int k, double lambda, int* __restrict__ out_pos) {
    extern __shared__ __attribute__((aligned(16))) float mm[];
    const int ld = dim + 1;
    float* qs = mm + 64 * ld;
    double* G = (double*)(mm + 64 * 385 + 384);               // [65][64]: rows 0..63 = X X^T (upper triangle), row 64 = q . x_j; then q . q
    const int64_t qi = blockIdx.x;
    for (int i = threadIdx.x; i < fetch_k * dim; i += 256) {
        const int r = i / dim, c = i - r * dim;
        const int64_t row = rows[qi * fetch_k + r];
        mm[r * ld + c] = (row >= 0 && row < n_rows) ? x[row * (int64_t)dpad + c] : 0.f;
    }
    for (int c = threadIdx.x; c < dim; c += 256) qs[c] = q[qi * dim + c];
    __syncthreads();
    const int n = fetch_k;
    const int n_tri = n * (n + 1) / 2, n_tasks = n_tri + n + 1;
    for (int p = threadIdx.x; p < n_tasks; p += 256) {
        const float *a, *b;
        double* dst;
        if (p < n_tri) {
            int i = 0, rem = p;
            while (rem >= n - i) { rem -= n - i; ++i; }
            const int j = i + rem;
            a = mm + i * ld; b = mm + j * ld; dst = G + i * 64 + j;
        } else if (p < n_tri + n) {
            const int j = p - n_tri;
            a = qs; b = mm + j * ld; dst = G + 64 * 64 + j;
        } else {
            a = qs; b = qs; dst = G + 65 * 64;
        }
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        int c = 0;
        for (; c + 4 <= dim; c += 4) {
            s0 = fma((double)a[c], (double)b[c], s0);
            s1 = fma((double)a[c + 1], (double)b[c + 1], s1);
            s2 = fma((double)a[c + 2], (double)b[c + 2], s2);
            s3 = fma((double)a[c + 3], (double)b[c + 3], s3);
        }
        for (; c < dim; ++c) s0 = fma((double)a[c], (double)b[c], s0);
        *dst = (s0 + s1) + (s2 + s3);
    }
    __syncthreads();
    if (threadIdx.x >= 64) return;
    const int lane = threadIdx.x;
    const int64_t row = lane < fetch_k ? rows[qi * fetch_k + lane] : -1;
    const int li = lane < fetch_k ? lane : 0;
    const double nx = sqrt(G[li * 64 + li]), nqq = sqrt(G[65 * 64]);
    const bool valid = row >= 0 && row < n_rows && nx == nx;          // as in k_mmr: a removed (NaN) row is absent
    double sim_q = G[64 * 64 + li] / (nx * nqq);
    if (!(sim_q == sim_q) || isinf(sim_q)) sim_q = 0.0;
    const int n_valid = __builtin_popcountll(__ballot(valid));
    const int want = k < n_valid ? k : n_valid;
    auto argmax = [&](double v, bool ok) -> int {
        double m = ok ? v : -INFINITY;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o));
        const unsigned long long eq = __ballot(ok && v == m);
        return eq ? __builtin_ctzll(eq) : -1;
    };
    bool picked = false;
    double red = -INFINITY;
    int sel = argmax(sim_q, valid);
    for (int t = 0; t < want && sel >= 0; ++t) {
        if (lane == 0) out_pos[qi * k + t] = sel;
        if (lane == sel) picked = true;
        if (t + 1 == want) break;
        const double ns = __shfl(nx, sel);
        const double d = li <= sel ? G[li * 64 + sel] : G[sel * 64 + li];
        double cs = d / (nx * ns);
        if (!(cs == cs) || isinf(cs)) cs = 0.0;
        red = fmax(red, cs);
        sel = argmax(lambda * sim_q - (1.0 - lambda) * red, valid && !picked);
    }
    for (int t = want + lane; t < k; t += 64) out_pos[qi * k + t] = -1;
}

// picks -> result rows / scores of rmu_index_search_mmr: out[qi, t] = candidate list entry pos[qi, t] (+ row_base), -1 where pos is -1
__global__ void k_take_picks(const int* __restrict__ pos, const int64_t* __restrict__ rows, const float* __restrict__ scores, int64_t nq,
                             int fetch_k, int k, int64_t row_base, int64_t* __restrict__ out_rows, float* __restrict__ out_scores) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq * k) return;
    const int64_t qi = i / k;
    const int p = pos ? pos[i] : (int)(i - qi * k);      // pos == nullptr: no selection, the first k candidates in score order
    const int64_t r = p >= 0 ? rows[qi * fetch_k + p] : -1;
    out_rows[i] = r >= 0 ? r + row_base : -1;
    out_scores[i] = p >= 0 ? scores[qi * fetch_k + p] : -INFINITY;
}

// ------------------------------------------------------------------------------------------------
// index
// ------------------------------------------------------------------------------------------------
struct rmu_index {
    int dim = 0, dpad = 0, metric = 0;
    int64_t n = 0, cap = 0, n_live = 0;
    float* x = nullptr;
    char* split = nullptr;          // fp16(64 x) image of x (screening pass), 768 B per row; nullptr = disabled
    float* nrm = nullptr;           // RMU_METRIC_L2SQ with an image: -2048 |x|^2 per row (NaN past the last row); exists iff split does
    float xnorm_max = 0.f;          // max row norm (bounds the screening error)
    float dx_max = 0.f;             // max row norm of (x - screening image): the measured rounding error
    unsigned stat_host[2] = {0, 0}; // landing pair of update_image_stats (|x|^2 max, |dx|^2 max of the rows just added)
    bool stat_pending = false;
    int64_t grow_count = 0;         // re-allocations of the corpus matrix (+ image) by rmu_index_add, and their wall time
    double grow_ms = 0.0;
    int64_t compact_count = 0;      // rmu_index_compact calls that dropped rows, and their wall time
    double compact_ms = 0.0;
    bool compact_inplace = false;   // RMU_OPT_COMPACT_INPLACE: compaction never re-allocates
    bool screen_enabled = true;     // RMU_OPT_SCREEN: searches may take the screening path (when `split` exists)
    bool wide_scan = false;         // RMU_OPT_WIDE_SCAN: exact searches run scan_wide_kernel whatever the width; no screening while set
    int ladder_ratio = 0, ladder_first = 0;   // RMU_OPT_LADDER_RATIO / _FIRST (0 = defaults; tools/ladder_sweep.py)
    bool screen_band = true;        // RMU_OPT_SCREEN_BAND: the ladder's merges also seed the lower edge of the sufficiency band (screen_enqueue)
    bool screen_spill = true;       // RMU_OPT_SCREEN_SPILL: seeded 8-wave launches spill passing lanes, rmu_sift_launch files them (screen_enqueue)
    int spill_cap = 0;              // RMU_OPT_SCREEN_SPILL_CAP: records per spill list (0 = kSpillCap)
    bool screen_refresh = false;    // RMU_OPT_SCREEN_REFRESH: every wave of a spill launch re-reads and refreshes its thresholds at every pair of tiles
                                    // (0, the default: only the waves that can use them -- 1.3-1.5 % of the headline: profiles/screen_refresh.md)
    int64_t screen_min_nq = 0;      // RMU_OPT_SCREEN_MIN_NQ: > 0 = screen every batch of at least this many queries, whatever the corpus size
    std::vector<uint8_t> alive;
    std::shared_mutex mu;
    // Streams on which scans of this index may still be running AFTER their call returned (a search handed a caller stream and device
    // buffers only enqueues: rmu_index_search's `drained == false`).  One event per stream, re-recorded behind each such search.  A
    // writer (growth, row removal, free) holds `mu` exclusively -- nothing new can start -- and waits for exactly these events instead of
    // the whole device (round 6: hipDeviceSynchronize breaks hipGraph captures of other threads, rmu_common.h).
    struct Reader { hipStream_t s; hipEvent_t ev; };
    std::vector<Reader> readers;
    std::mutex readers_mu;
};

// (shared lock held) the scans just enqueued on `s` stay in flight behind the caller's back
static void mark_reader(rmu_index* idx, hipStream_t s) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess) { (void)hipGetLastError(); return; }
    if (st != hipStreamCaptureStatusNone) return;   // a search captured into the caller's graph: replays are the caller's to order against writers
    std::lock_guard<std::mutex> g(idx->readers_mu);
    for (auto& r : idx->readers)
        if (r.s == s) { (void)hipEventRecord(r.ev, s); return; }
    if (idx->readers.size() >= 64) {                // streams come and go (a thread per request): drop the marks whose work has ended
        size_t w = 0;
        for (auto& r : idx->readers) {
            if (hipEventQuery(r.ev) == hipSuccess) (void)hipEventDestroy(r.ev);
            else idx->readers[w++] = r;
        }
        (void)hipGetLastError();
        idx->readers.resize(w);
    }
    hipEvent_t ev = nullptr;
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); (void)hipStreamSynchronize(s); return; }
    if (hipEventRecord(ev, s) != hipSuccess) { (void)hipGetLastError(); (void)hipEventDestroy(ev); (void)hipStreamSynchronize(s); return; }
    idx->readers.push_back({s, ev});
}
// (exclusive lock held) host-side wait for every scan still in flight; `on` != nullptr: order stream `on` behind them instead (no host wait)
static int wait_readers(rmu_index* idx, hipStream_t on = nullptr) {
    std::lock_guard<std::mutex> g(idx->readers_mu);
    for (auto& r : idx->readers) {
        const hipError_t e = on ? hipStreamWaitEvent(on, r.ev, 0) : hipEventSynchronize(r.ev);
        if (e != hipSuccess) return rmu_fail(RMU_E_HIP, std::string("waiting for the scans in flight: ") + hipGetErrorString(e));
    }
    return RMU_OK;
}

// The scans' LDS-DMA rings run past the last row: the exact scan reads whole 128-row tiles; the screening scan (scan_screen_lean3_kernel)
// looks four 32-row tiles ahead of the tile it computes and does not clamp, i.e. it touches up to (ceil(n / 32) + 4) * 32 - n <= 159 rows
// past row n of the image.  Keep this many allocated (zero-filled) rows past the capacity of both matrices.
static const int64_t kSlackRows = 256;
static_assert(kSlackRows >= 160, "scan_screen_lean3_kernel's unclamped look-ahead");
// ... wide rows (scan_wide.hip streams them in 32- or 16-float chunks): the next multiple of 64 floats, i.e. of 256 bytes (rmu_compact.hip)
static int pad_dim(int d) { return d <= 192 ? 192 : (d <= 384 ? 384 : (d <= RMU_MAX_DIM ? 768 : (d <= RMU_MAX_DIM_WIDE ? (d + 63) / 64 * 64 : -1))); }
// L2SQ rows carry -|x|^2 in one extra column (see k_l2_aug_rows); there is no wide L2 index
static int pad_dim_metric(int d, int metric) {
    if (metric == RMU_METRIC_L2SQ) return d + 1 <= RMU_MAX_DIM ? pad_dim(d + 1) : -1;
    return pad_dim(d);
}

extern "C" int rmu_index_create(rmu_index_t** out, int dim, int metric, int64_t capacity_hint) {
    RMU_ENTRY();
    if (!out) return rmu_fail(RMU_E_INVALID, "rmu_index_create: out is null");
    if (dim < 1 || dim > RMU_MAX_DIM_WIDE) return rmu_fail(RMU_E_INVALID, "rmu_index_create: dim must be in [1, 3072]");
    if (metric != RMU_METRIC_IP && metric != RMU_METRIC_COSINE && metric != RMU_METRIC_L2SQ)
        return rmu_fail(RMU_E_INVALID, "rmu_index_create: metric must be RMU_METRIC_IP, RMU_METRIC_COSINE or RMU_METRIC_L2SQ");
    if (pad_dim_metric(dim, metric) < 0)
        return rmu_fail(RMU_E_INVALID, dim <= RMU_MAX_DIM ? "rmu_index_create: RMU_METRIC_L2SQ needs one spare column: dim must be <= 767"
                                                      : "rmu_index_create: a wide index (dim > 768) is RMU_METRIC_IP or RMU_METRIC_COSINE: RMU_METRIC_L2SQ (L2) "
                                                        "rows are at most 767 dimensions");
    int rc = g_tls.ensure_stream();
    if (rc) return rmu_fail(rc, "rmu_index_create: stream");
    auto* idx = new (std::nothrow) rmu_index();
    if (!idx) return rmu_fail(RMU_E_OOM, "rmu_index_create: host alloc");
    idx->dim = dim;
    idx->dpad = pad_dim_metric(dim, metric);
    idx->metric = metric;
    int64_t cap = capacity_hint > 0 ? capacity_hint : 4096;
    hipError_t e = hipMalloc((void**)&idx->x, (size_t)(cap + kSlackRows) * idx->dpad * sizeof(float));
    if (e != hipSuccess) { delete idx; return rmu_fail(RMU_E_OOM, "rmu_index_create: hipMalloc"); }
    // zero fill ON OUR STREAM and wait: a null-stream hipMemset is asynchronous to the host and is not ordered
    // with a hipStreamNonBlocking stream, so it could land after (and wipe) the first rows uploaded on it
    if (hipMemsetAsync(idx->x, 0, (size_t)(cap + kSlackRows) * idx->dpad * sizeof(float), g_tls.stream) != hipSuccess ||
        hipStreamSynchronize(g_tls.stream) != hipSuccess) {
        (void)hipFree(idx->x);
        delete idx;
        return rmu_fail(RMU_E_HIP, "rmu_index_create: zero fill");
    }
    idx->cap = cap;
    // screening image (+50% corpus memory): 384-wide rows only; RMU_SCREEN=0 disables
    static const bool screen_on = !(rmu_env_kill("RMU_SCREEN") && atoi(rmu_env_kill("RMU_SCREEN")) == 0);
    // (round 5) ... and the native L2 index at dim 384 (rows 768 floats apart: 384 + the -|x|^2 column, padded), with the row norms beside it
    const bool l2 = metric == RMU_METRIC_L2SQ;
    if (screen_on && dim == 384 && (idx->dpad == 384 || l2)) {
        if (hipMalloc((void**)&idx->split, (size_t)(cap + kSlackRows) * RMU_IMG_ROW_BYTES) != hipSuccess) {
            idx->split = nullptr;   // not fatal: exact path only
            (void)hipGetLastError();
        } else if (l2 && hipMalloc((void**)&idx->nrm, (size_t)(cap + kSlackRows) * sizeof(float)) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(idx->split);
            idx->split = nullptr; idx->nrm = nullptr;
        } else {
            (void)hipMemsetAsync(idx->split, 0, (size_t)(cap + kSlackRows) * RMU_IMG_ROW_BYTES, g_tls.stream);
            if (idx->nrm) (void)hipMemsetAsync(idx->nrm, 0xFF, (size_t)(cap + kSlackRows) * sizeof(float), g_tls.stream);   // NaN: never a candidate
            (void)hipStreamSynchronize(g_tls.stream);
        }
    }
    *out = idx;
    return RMU_OK;
}

extern "C" int rmu_index_free(rmu_index_t* idx) {
    RMU_ENTRY();
    if (!idx) return RMU_OK;
    {
        std::unique_lock<std::shared_mutex> lk(idx->mu);
        (void)wait_readers(idx);          // scans still in flight on callers' streams (everything else ended under the shared lock)
        if (idx->x) (void)hipFree(idx->x);
        if (idx->split) (void)hipFree(idx->split);
        if (idx->nrm) (void)hipFree(idx->nrm);
        idx->x = nullptr;
        idx->split = nullptr;
        idx->nrm = nullptr;
        for (auto& r : idx->readers) (void)hipEventDestroy(r.ev);
        idx->readers.clear();
    }
    delete idx;
    return RMU_OK;
}

extern "C" int rmu_index_size(rmu_index_t* idx, int64_t* n_rows) {
    if (!idx || !n_rows) return rmu_fail(RMU_E_INVALID, "rmu_index_size: null");
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    *n_rows = idx->n;
    return RMU_OK;
}
extern "C" int rmu_index_stat(rmu_index_t* idx, int what, double* out) {
    if (!idx || !out) return rmu_fail(RMU_E_INVALID, "rmu_index_stat: null");
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    switch (what) {
        case RMU_STAT_CAPACITY: *out = (double)idx->cap; break;
        case RMU_STAT_GROW_COUNT: *out = (double)idx->grow_count; break;
        case RMU_STAT_GROW_MS: *out = idx->grow_ms; break;
        case RMU_STAT_LIVE_ROWS: *out = (double)idx->n_live; break;
        case RMU_STAT_COMPACT_COUNT: *out = (double)idx->compact_count; break;
        case RMU_STAT_COMPACT_MS: *out = idx->compact_ms; break;
        default: return rmu_fail(RMU_E_INVALID, "rmu_index_stat: unknown statistic");
    }
    return RMU_OK;
}
extern "C" int rmu_index_dim(rmu_index_t* idx, int* dim) {
    if (!idx || !dim) return rmu_fail(RMU_E_INVALID, "rmu_index_dim: null");
    *dim = idx->dim;
    return RMU_OK;
}

static int grow(rmu_index* idx, int64_t need) {
    if (need <= idx->cap) return RMU_OK;
    const auto t0 = std::chrono::steady_clock::now();
    struct Tick {
        rmu_index* i; std::chrono::steady_clock::time_point t;
        ~Tick() { i->grow_count++; i->grow_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); }
    } tick{idx, t0};
    int64_t cap = idx->cap;
    while (cap < need) cap = cap + cap / 2 + 1024;
    float* nx = nullptr;
    if (hipMalloc((void**)&nx, (size_t)(cap + kSlackRows) * idx->dpad * sizeof(float)) != hipSuccess) {
        cap = need;  // retry with the exact size before giving up
        if (hipMalloc((void**)&nx, (size_t)(cap + kSlackRows) * idx->dpad * sizeof(float)) != hipSuccess)
            return rmu_fail(RMU_E_OOM, "rmu_index_add: hipMalloc for growth");
    }
    // nobody may still be scanning the old matrix when it is freed below: searches on internal streams ended under the shared lock, the
    // ones left in flight on callers' streams are waited for one by one -- never the whole device (rmu_common.h: captures)
    int wrc = wait_readers(idx);
    if (wrc) { (void)rmu_free(nx); return wrc; }
    hipStream_t s = g_tls.stream;     // same stream as the uploads that follow (see rmu_index_create)
    RMU_HIP_TRY(hipMemsetAsync(nx + idx->n * idx->dpad, 0, (size_t)(cap + kSlackRows - idx->n) * idx->dpad * sizeof(float), s));
    if (idx->n)
        RMU_HIP_TRY(hipMemcpyAsync(nx, idx->x, (size_t)idx->n * idx->dpad * sizeof(float), hipMemcpyDeviceToDevice, s));
    RMU_HIP_TRY(hipStreamSynchronize(s));
    if (idx->split) {
        char* ns = nullptr;
        float* nn = nullptr;
        const size_t rowb = RMU_IMG_ROW_BYTES;
        bool got = hipMalloc((void**)&ns, (size_t)(cap + kSlackRows) * rowb) == hipSuccess;
        if (got && idx->nrm && hipMalloc((void**)&nn, (size_t)(cap + kSlackRows) * sizeof(float)) != hipSuccess) {
            (void)rmu_free(ns);
            got = false;
        }
        if (got) {
            RMU_HIP_TRY(hipMemsetAsync(ns + idx->n * rowb, 0, (size_t)(cap + kSlackRows - idx->n) * rowb, s));
            if (idx->n) RMU_HIP_TRY(hipMemcpyAsync(ns, idx->split, (size_t)idx->n * rowb, hipMemcpyDeviceToDevice, s));
            if (nn) {
                RMU_HIP_TRY(hipMemsetAsync(nn + idx->n, 0xFF, (size_t)(cap + kSlackRows - idx->n) * sizeof(float), s));
                if (idx->n) RMU_HIP_TRY(hipMemcpyAsync(nn, idx->nrm, (size_t)idx->n * sizeof(float), hipMemcpyDeviceToDevice, s));
            }
            RMU_HIP_TRY(hipStreamSynchronize(s));
            (void)rmu_free(idx->split);
            if (idx->nrm) (void)rmu_free(idx->nrm);
            idx->split = ns;
            idx->nrm = nn;
        } else {
            (void)hipGetLastError();
            (void)rmu_free(idx->split);   // no room for the screening image: exact path only from now on
            if (idx->nrm) (void)rmu_free(idx->nrm);
            idx->split = nullptr;
            idx->nrm = nullptr;
        }
    }
    (void)rmu_free(idx->x);
    idx->x = nx;
    idx->cap = cap;
    return RMU_OK;
}

extern "C" int rmu_index_reserve(rmu_index_t* idx, int64_t rows) {
    RMU_ENTRY();
    if (!idx || rows < 0) return rmu_fail(RMU_E_INVALID, "rmu_index_reserve: bad argument");
    if (rows > 0xFFFFFFF0ll) return rmu_fail(RMU_E_INVALID, "rmu_index_reserve: row ids are 32-bit inside the scan");
    int rc = g_tls.ensure_stream();
    if (rc) return rmu_fail(rc, "rmu_index_reserve: stream");
    std::unique_lock<std::shared_mutex> lk(idx->mu);
    return grow(idx, rows);           // (rmu_index_add's geometric policy: a caller that reserves round by round does not re-allocate every round)
}

// after `n` rows at `dst` were converted into the screening image: |x|max and the measured image error |dx|max of those rows.
// ENQUEUES only (two reductions into one 8-byte device pair + one 8-byte copy to idx->stat_host): the caller's own final
// stream synchronisation covers it, then fold_image_stats() folds the pair into the index -- one host round trip per
// rmu_index_add instead of three (the reference inserts in 1000-document calls, server/RAGHelper.py:423-434).
static int update_image_stats(rmu_index_t* idx, const float* dst, int64_t n, hipStream_t s, float* nrm_out = nullptr) {
    RmuDevBuf& nb = g_tls.nrm;
    if (nb.ensure((size_t)n * sizeof(float) + 16)) return rmu_fail(RMU_E_OOM, "rmu_index_add: norm workspace");
    unsigned* mx = (unsigned*)((char*)nb.p + (size_t)n * sizeof(float));
    RMU_HIP_TRY(hipMemsetAsync(mx, 0, 2 * sizeof(unsigned), s));
    if (idx->metric == RMU_METRIC_L2SQ) {      // |x|^2 is the augmented column (k_l2_aug_rows), not the norm of the augmented row
        hipLaunchKernelGGL(k_l2_nrm, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dst, idx->dpad, idx->dim, n, nrm_out, (float*)nb.p);
        hipLaunchKernelGGL(k_max_norm2, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float*)nb.p, n, mx);
    } else if (idx->metric != RMU_METRIC_COSINE) {
        hipLaunchKernelGGL(k_row_norm, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, const_cast<float*>(dst), idx->dpad, n, 0, (float*)nb.p);
        hipLaunchKernelGGL(k_max_norm2, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float*)nb.p, n, mx);
    }
    int rc = rmu_img_err_launch(dst, n, (float*)nb.p, s, idx->dpad);
    if (rc) return rmu_fail(rc, "rmu_index_add: image error");
    hipLaunchKernelGGL(k_max_norm2, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float*)nb.p, n, mx + 1);
    RMU_HIP_TRY(hipGetLastError());
    RMU_HIP_TRY(hipMemcpyAsync(idx->stat_host, mx, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, s));
    idx->stat_pending = true;
    return RMU_OK;
}

// rows [r0, r0 + n) of idx->x (final form: normalised / augmented) -> screening image (+ row norms of an L2 index) + statistics.  Enqueues only.
static int build_image(rmu_index_t* idx, int64_t r0, int64_t n, hipStream_t s) {
    if (!idx->split) return RMU_OK;
    const float* rows = idx->x + r0 * (int64_t)idx->dpad;
    int rc = rmu_split_launch(rows, idx->split + (size_t)r0 * RMU_IMG_ROW_BYTES, n, s, idx->dpad, 64.0f);
    if (rc) return rmu_fail(rc, "rmu_index_add: split image");
    return update_image_stats(idx, rows, n, s, idx->nrm ? idx->nrm + r0 : nullptr);
}

// after the stream that ran update_image_stats was synchronised
static void fold_image_stats(rmu_index_t* idx) {
    if (!idx->stat_pending) return;
    idx->stat_pending = false;
    float f;
    if (idx->metric == RMU_METRIC_COSINE) {
        idx->xnorm_max = 1.0f;
    } else {
        memcpy(&f, &idx->stat_host[0], 4);
        f = sqrtf(f);
        if (f > idx->xnorm_max) idx->xnorm_max = f;
    }
    memcpy(&f, &idx->stat_host[1], 4);
    f = sqrtf(f) * 1.0001f;
    if (f > idx->dx_max) idx->dx_max = f;
}

extern "C" int rmu_index_add(rmu_index_t* idx, const float* vecs, int64_t n, int is_device, int64_t* first_row) {
    RMU_ENTRY();
    if (!idx || (!vecs && n > 0) || n < 0) return rmu_fail(RMU_E_INVALID, "rmu_index_add: bad argument");
    int rc = g_tls.ensure_stream();
    if (rc) return rmu_fail(rc, "rmu_index_add: stream");
    std::unique_lock<std::shared_mutex> lk(idx->mu);
    if (first_row) *first_row = idx->n;
    if (n == 0) return RMU_OK;
    if (idx->n + n > 0xFFFFFFF0ll) return rmu_fail(RMU_E_INVALID, "rmu_index_add: row ids are 32-bit inside the scan");
    rc = grow(idx, idx->n + n);
    if (rc) return rc;
    float* dst = idx->x + idx->n * (int64_t)idx->dpad;
    hipStream_t s = g_tls.stream;
    const hipMemcpyKind kind = is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (idx->dpad == idx->dim)
        RMU_HIP_TRY(hipMemcpyAsync(dst, vecs, (size_t)n * idx->dim * sizeof(float), kind, s));
    else
        RMU_HIP_TRY(hipMemcpy2DAsync(dst, (size_t)idx->dpad * sizeof(float), vecs, (size_t)idx->dim * sizeof(float),
                                 (size_t)idx->dim * sizeof(float), (size_t)n, kind, s));
    if (idx->metric == RMU_METRIC_COSINE) {
        const int wpb = 4;
        hipLaunchKernelGGL(k_row_norm, dim3((unsigned)((n + wpb - 1) / wpb)), dim3(64 * wpb), 0, s, dst, idx->dpad, n, 1,
                           (float*)nullptr);
        RMU_HIP_TRY(hipGetLastError());
    }
    if (idx->metric == RMU_METRIC_L2SQ) {
        hipLaunchKernelGGL(k_l2_aug_rows, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, dst, idx->dpad, idx->dim, n);
        RMU_HIP_TRY(hipGetLastError());
    }
    rc = build_image(idx, idx->n, n, s);
    if (rc) return rc;
    RMU_HIP_TRY(hipStreamSynchronize(s));
    fold_image_stats(idx);
    idx->alive.resize((size_t)(idx->n + n), 1);
    idx->n += n;
    idx->n_live += n;
    return RMU_OK;
}

extern "C" int rmu_index_remove_rows(rmu_index_t* idx, const int64_t* rows, int64_t n, int64_t* n_removed) {
    RMU_ENTRY();
    if (!idx || (!rows && n > 0) || n < 0) return rmu_fail(RMU_E_INVALID, "rmu_index_remove_rows: bad argument");
    int rc = g_tls.ensure_stream();
    if (rc) return rmu_fail(rc, "rmu_index_remove_rows: stream");
    std::unique_lock<std::shared_mutex> lk(idx->mu);
    std::vector<int64_t> todo;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t r = rows[i];
        if (r < 0 || r >= idx->n) return rmu_fail(RMU_E_INVALID, "rmu_index_remove_rows: row out of range");
        if (idx->alive[(size_t)r]) { idx->alive[(size_t)r] = 0; todo.push_back(r); }
    }
    if (n_removed) *n_removed = (int64_t)todo.size();
    if (todo.empty()) return RMU_OK;
    RmuDevBuf& b = g_tls.in_r;
    if (b.ensure(todo.size() * sizeof(int64_t))) return rmu_fail(RMU_E_OOM, "rmu_index_remove_rows: workspace");
    hipStream_t s = g_tls.stream;
    rc = wait_readers(idx, s);        // the poison kernels are ordered behind the scans still in flight on callers' streams
    if (rc) return rc;
    RMU_HIP_TRY(hipMemcpyAsync(b.p, todo.data(), todo.size() * sizeof(int64_t), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_poison_rows, dim3((unsigned)todo.size()), dim3(128), 0, s, idx->x, idx->dpad,
                       (const int64_t*)b.p, (int64_t)todo.size());
    if (idx->split)   // fp32 NaN pattern = one fp16 NaN per pair: every screening score of the row is NaN as well
        hipLaunchKernelGGL(k_poison_rows, dim3((unsigned)todo.size()), dim3(128), 0, s, (float*)idx->split, RMU_IMG_ROW_BYTES / 4,
                           (const int64_t*)b.p, (int64_t)todo.size());
    RMU_HIP_TRY(hipGetLastError());
    RMU_HIP_TRY(hipStreamSynchronize(s));
    idx->n_live -= (int64_t)todo.size();
    return RMU_OK;
}

// Drop the tombstoned rows (rmu.h).  The live rows from the first dead one on are gathered forward (rmu_compact.hip), array by array:
// out of place into allocations of max(4096, n_live + n_live / 8 + 1024) rows (+ slack) -- one array's old and new allocation coexist at a
// time, as in grow() -- or in place through a staging buffer (RMU_OPT_COMPACT_INPLACE, a new capacity that would not be smaller, or a failed
// allocation).  Afterwards the index is what a fresh index of the live rows would hold: rows past n_live zero (x, image) / NaN (norms).
extern "C" int rmu_index_compact(rmu_index_t* idx, int64_t* old_to_new, int64_t map_len, int64_t* n_after) {
    RMU_ENTRY();
    if (!idx || !n_after || (old_to_new && map_len < 0)) return rmu_fail(RMU_E_INVALID, "rmu_index_compact: bad argument");
    int rc = g_tls.ensure_stream();
    if (rc) return rmu_fail(rc, "rmu_index_compact: stream");
    std::unique_lock<std::shared_mutex> lk(idx->mu);
    const int64_t n = idx->n, n_live = idx->n_live;
    if (old_to_new && map_len < n) return rmu_fail(RMU_E_INVALID, "rmu_index_compact: map_len is smaller than the index's row count");
    const auto t0 = std::chrono::steady_clock::now();
    // the map, and the source row of every new row from the first dead row on (branch-free: tombstones fall anywhere)
    const uint8_t* alive = idx->alive.data();
    const uint8_t* d0 = n ? (const uint8_t*)memchr(alive, 0, (size_t)n) : nullptr;
    const int64_t first = d0 ? (int64_t)(d0 - alive) : n;
    if (old_to_new) {
        for (int64_t r = 0; r < first; ++r) old_to_new[r] = r;
        for (int64_t r = first, j = first; r < n; ++r) {
            old_to_new[r] = alive[r] ? j : -1;
            j += alive[r];
        }
        for (int64_t r = n; r < map_len; ++r) old_to_new[r] = -1;
    }
    *n_after = n;
    if (first == n) return RMU_OK;                         // nothing dead: nothing moves, nothing is re-allocated
    std::vector<u32> src((size_t)(n_live - first) + 1);
    for (int64_t r = first, i = 0; r < n; ++r) {
        src[(size_t)i] = (u32)r;
        i += alive[r];
    }
    src.pop_back();
    struct Tick {
        rmu_index* i; std::chrono::steady_clock::time_point t;
        ~Tick() { i->compact_count++; i->compact_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); }
    } tick{idx, t0};
    // scans still in flight on callers' streams read the rows about to move (and maybe the allocations about to be freed)
    rc = wait_readers(idx);
    if (rc) return rc;
    hipStream_t s = g_tls.stream;
    RmuDevBuf& bs = g_tls.in_r;
    if (!src.empty()) {
        if (bs.ensure(src.size() * sizeof(u32))) return rmu_fail(RMU_E_OOM, "rmu_index_compact: source list workspace");
        RMU_HIP_TRY(hipMemcpyAsync(bs.p, src.data(), src.size() * sizeof(u32), hipMemcpyHostToDevice, s));
    }
    const u32* d_src = (const u32*)bs.p;
    const int64_t new_cap = std::max<int64_t>(4096, n_live + n_live / 8 + 1024);
    const size_t kStagingBytes = (size_t)64 << 20;
    void* staging = nullptr;
    auto get_staging = [&]() -> bool {
        if (!staging && hipMalloc(&staging, kStagingBytes) != hipSuccess) { (void)hipGetLastError(); staging = nullptr; }
        return staging != nullptr;
    };
    struct Arr { void** base; int64_t row_bytes; int fill; };
    Arr arrs[3] = {{(void**)&idx->x, (int64_t)idx->dpad * (int64_t)sizeof(float), 0},
                   {(void**)&idx->split, RMU_IMG_ROW_BYTES, 0},
                   {(void**)&idx->nrm, (int64_t)sizeof(float), 0xFF}};   // NaN norms: never a candidate
    bool oop = !idx->compact_inplace && new_cap < idx->cap;
    if (!oop && !get_staging()) return rmu_fail(RMU_E_OOM, "rmu_index_compact: staging buffer (the index is unchanged)");
    hipError_t e = hipSuccess;
    for (int a = 0; a < 3 && e == hipSuccess; ++a) {
        if (!*arrs[a].base) continue;
        const Arr& A = arrs[a];
        if (oop) {
            e = rmu_compact_array(A.base, A.row_bytes, A.fill, n, n_live, first, d_src, new_cap + kSlackRows, nullptr, 0, s);
            if (e != hipErrorOutOfMemory) continue;
            e = hipSuccess;
            if (a == 0) {                                  // the matrix did not fit twice: the whole call goes in place
                oop = false;
                if (!get_staging()) return rmu_fail(RMU_E_OOM, "rmu_index_compact: staging buffer (the index is unchanged)");
            } else if (!get_staging()) {                   // the matrix has moved; no room for the image either way: exact path only
                (void)hipStreamSynchronize(s);             // (as grow() does when the image does not fit)
                (void)rmu_free(idx->split);
                if (idx->nrm) (void)rmu_free(idx->nrm);
                idx->split = nullptr;
                idx->nrm = nullptr;
                break;
            }
        }
        e = rmu_compact_array(A.base, A.row_bytes, A.fill, n, n_live, first, d_src, 0, staging, kStagingBytes, s);
    }
    const hipError_t es = hipStreamSynchronize(s);
    if (staging) (void)rmu_free(staging);
    if (e != hipSuccess || es != hipSuccess)
        return rmu_fail(RMU_E_HIP, std::string("rmu_index_compact: ") + hipGetErrorString(e != hipSuccess ? e : es));
    if (oop) idx->cap = new_cap;
    idx->n = n_live;
    idx->alive.assign((size_t)n_live, 1);
    *n_after = n_live;
    return RMU_OK;
}

extern "C" int rmu_index_get_rows(rmu_index_t* idx, const int64_t* rows, int64_t n, float* out_host) {
    RMU_ENTRY();
    if (!idx || (!rows && n > 0) || (!out_host && n > 0) || n < 0)
        return rmu_fail(RMU_E_INVALID, "rmu_index_get_rows: bad argument");
    if (n == 0) return RMU_OK;
    int rc = g_tls.ensure_stream();
    if (rc) return rmu_fail(rc, "rmu_index_get_rows: stream");
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    for (int64_t i = 0; i < n; ++i)
        if (rows[i] < 0 || rows[i] >= idx->n) return rmu_fail(RMU_E_INVALID, "rmu_index_get_rows: row out of range");
    RmuDevBuf& br = g_tls.in_r;
    RmuDevBuf& bo = g_tls.out_s;
    if (br.ensure((size_t)n * sizeof(int64_t)) || bo.ensure((size_t)n * idx->dim * sizeof(float)))
        return rmu_fail(RMU_E_OOM, "rmu_index_get_rows: workspace");
    hipStream_t s = g_tls.stream;
    RMU_HIP_TRY(hipMemcpyAsync(br.p, rows, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)n), dim3(128), 0, s, idx->x, idx->dpad, idx->dim,
                       (const int64_t*)br.p, n, (float*)bo.p);
    RMU_HIP_TRY(hipGetLastError());
    RMU_HIP_TRY(hipMemcpyAsync(out_host, bo.p, (size_t)n * idx->dim * sizeof(float), hipMemcpyDeviceToHost, s));
    RMU_HIP_TRY(hipStreamSynchronize(s));
    return RMU_OK;
}

static void launch_mmr(const rmu_index* idx, const float* dq, const int64_t* dr, int64_t nq, int fetch_k, int k, double lambda_mult, int* dout,
                       hipStream_t s) {
    static const bool lds_off = rmu_env("RMU_MMR_LDS") && atoi(rmu_env("RMU_MMR_LDS")) == 0;
    if (idx->dim <= 384 && nq <= 65535 && !lds_off) {          // one workgroup per query, candidates staged in LDS (bit-identical picks: tests/test_mmr_regimes_gpu.py)
        // rows [64][dim + 1] + q [dim] at the head of a (64 * 385 + 384)-float area, then the fp64 Gram block [65][64] + 1
        const size_t lds = (size_t)(64 * 385 + 384) * sizeof(float) + (size_t)(65 * 64 + 1) * sizeof(double);
        static const hipError_t attr_rc = hipFuncSetAttribute((const void*)k_mmr_lds, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                              (64 * 385 + 384) * 4 + (65 * 64 + 1) * 8);
        (void)attr_rc;
        hipLaunchKernelGGL(k_mmr_lds, dim3((unsigned)nq), dim3(256), lds, s, idx->x, idx->dpad, idx->dim, idx->n, dq, dr, nq, fetch_k, k, lambda_mult, dout);
    } else {
        hipLaunchKernelGGL(k_mmr, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, s, idx->x, idx->dpad, idx->dim, idx->n, dq, dr, nq, fetch_k,
                           k, lambda_mult, dout);
    }
}

extern "C" int rmu_index_mmr(rmu_index_t* idx, const float* q, int64_t nq, const int64_t* rows, int fetch_k, int k,
                             double lambda_mult, unsigned flags, int32_t* out_pos) {
    RMU_ENTRY();
    if (!idx || !q || !rows || !out_pos) return rmu_fail(RMU_E_INVALID, "rmu_index_mmr: null pointer");
    if (nq < 1 || fetch_k < 1 || fetch_k > 64 || k < 1) return rmu_fail(RMU_E_INVALID, "rmu_index_mmr: nq >= 1, fetch_k in [1, 64], k >= 1");
    Tls& t = g_tls;
    int rc = t.ensure_stream();
    if (rc) return rmu_fail(rc, "rmu_index_mmr: stream");
    hipStream_t s = t.stream;
    const bool q_dev = flags & RMU_F_Q_DEVICE, io_dev = flags & RMU_F_OUT_DEVICE;
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    const float* dq = q;
    const int64_t* dr = rows;
    int* dout = (int*)out_pos;
    if (!q_dev) {
        if (t.q.ensure((size_t)nq * idx->dim * sizeof(float))) return rmu_fail(RMU_E_OOM, "rmu_index_mmr: q workspace");
        RMU_HIP_TRY(hipMemcpyAsync(t.q.p, q, (size_t)nq * idx->dim * sizeof(float), hipMemcpyHostToDevice, s));
        dq = (const float*)t.q.p;
    }
    if (!io_dev) {
        if (t.in_r.ensure((size_t)nq * fetch_k * sizeof(int64_t)) || t.out_r.ensure((size_t)nq * k * sizeof(int)))
            return rmu_fail(RMU_E_OOM, "rmu_index_mmr: workspace");
        RMU_HIP_TRY(hipMemcpyAsync(t.in_r.p, rows, (size_t)nq * fetch_k * sizeof(int64_t), hipMemcpyHostToDevice, s));
        dr = (const int64_t*)t.in_r.p;
        dout = (int*)t.out_r.p;
    }
    launch_mmr(idx, dq, dr, nq, fetch_k, k, lambda_mult, dout, s);
    RMU_HIP_TRY(hipGetLastError());
    if (!io_dev) RMU_HIP_TRY(hipMemcpyAsync(out_pos, dout, (size_t)nq * k * sizeof(int), hipMemcpyDeviceToHost, s));
    RMU_HIP_TRY(hipStreamSynchronize(s));
    return RMU_OK;
}

// dense top-fetch_k + greedy selection of `nq` queries (host or device fp32 [nq, dim]), first half: everything is enqueued on stream s and the
// results are left on the device, *d_rows_out = rows [nq, k] int64 (+ row_base) with the scores [nq, k] fp32 right behind them (one contiguous
// block of the thread's workspace).  `lk` comes back holding the index's shared lock: the selection kernel reads the corpus matrix behind the
// search's reader mark, so the caller keeps the lock until it has drained s.  lambda_mult < 0: no selection -- the top-k (k <= fetch_k) in score
// order, as rmu_index_search returns them.  expect_rows >= 0 (the hybrid call, rrf_fuse.hip): the index must hold exactly that many rows, checked
// under the lock before anything is enqueued.
static int search_mmr_enqueue(rmu_index_t* idx, const float* q, bool q_dev, int64_t nq, int fetch_k, int k, double lambda_mult, int64_t row_base,
                              int64_t expect_rows, hipStream_t s, const char* who, std::shared_lock<std::shared_mutex>& lk, int64_t** d_rows_out) {
    Tls& t = g_tls;
    const size_t nf = (size_t)nq * fetch_k, nk = (size_t)nq * k;
    // candidate scores / rows, the raw queries (the search normalises its own copy for COSINE), picks, and the results (rows | scores)
    if (t.mm_s.ensure(nf * sizeof(float)) || t.mm_r.ensure(nf * sizeof(int64_t)) || t.mm_q.ensure((size_t)nq * idx->dim * sizeof(float)) ||
        t.mm_p.ensure(nk * (sizeof(int) + sizeof(int64_t) + sizeof(float))))
        return rmu_fail(RMU_E_OOM, std::string(who) + ": workspace");
    int64_t* d_rows = (int64_t*)t.mm_p.p;
    float* d_sc = (float*)(d_rows + nk);
    int* d_pos = (int*)(d_sc + nk);
    if (expect_rows >= 0) {
        std::shared_lock<std::shared_mutex> chk(idx->mu);
        if (idx->n != expect_rows)
            return rmu_fail(RMU_E_INVALID, std::string(who) + ": the dense key table (" + std::to_string(expect_rows) + " keys) and the index (" +
                                           std::to_string(idx->n) + " rows) are out of step");
    }
    // (round 5: every stream operation of the one-query path is ~4.4 us of dependent-kernel boundary.)  No selection and fetch_k == k: the
    // search writes the result rows (row_base applied) and scores where the caller reads them -- no k_take_picks launch.
    const bool direct = lambda_mult < 0.0 && fetch_k == k;
    // the search on the given stream, results left on the device (no synchronisation inside)
    int rc = direct ? rmu_index_search(idx, q, nq, k, RMU_F_OUT_DEVICE | (q_dev ? RMU_F_Q_DEVICE : 0u), row_base, d_sc, d_rows, (uint64_t)(uintptr_t)s)
                    : rmu_index_search(idx, q, nq, fetch_k, RMU_F_OUT_DEVICE | (q_dev ? RMU_F_Q_DEVICE : 0u), 0, (float*)t.mm_s.p, (int64_t*)t.mm_r.p,
                                       (uint64_t)(uintptr_t)s);
    if (rc) return rc;
    lk = std::shared_lock<std::shared_mutex>(idx->mu);
    if (!direct) {
        const float* dq = q;
        if (!q_dev && lambda_mult >= 0.0) {
            RMU_HIP_TRY(hipMemcpyAsync(t.mm_q.p, q, (size_t)nq * idx->dim * sizeof(float), hipMemcpyHostToDevice, s));
            dq = (const float*)t.mm_q.p;
        }
        if (lambda_mult >= 0.0) launch_mmr(idx, dq, (const int64_t*)t.mm_r.p, nq, fetch_k, k, lambda_mult, d_pos, s);
        hipLaunchKernelGGL(k_take_picks, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, s, lambda_mult >= 0.0 ? (const int*)d_pos : (const int*)nullptr,
                           (const int64_t*)t.mm_r.p, (const float*)t.mm_s.p, nq, fetch_k, k, row_base, d_rows, d_sc);
        RMU_HIP_TRY(hipGetLastError());
    }
    *d_rows_out = d_rows;
    return RMU_OK;
}

// ... and the second half: HOST results; drains s.
static int search_mmr_on(rmu_index_t* idx, const float* q, bool q_dev, int64_t nq, int fetch_k, int k, double lambda_mult, int64_t row_base,
                         int64_t* out_rows, float* out_scores, hipStream_t s, const char* who) {
    Tls& t = g_tls;
    const size_t nk = (size_t)nq * k;
    if (t.hpin.ensure(nk * (sizeof(int64_t) + sizeof(float)))) return rmu_fail(RMU_E_OOM, std::string(who) + ": pinned result buffer");
    std::shared_lock<std::shared_mutex> lk;
    int64_t* d_rows = nullptr;
    const int rc = search_mmr_enqueue(idx, q, q_dev, nq, fetch_k, k, lambda_mult, row_base, -1, s, who, lk, &d_rows);
    if (rc) return rc;
    // rows | scores are contiguous on the device: ONE copy into pinned memory (a copy into the caller's pageable arrays is staged by the
    // runtime, one staging round per call), split on the host behind the synchronisation
    RMU_HIP_TRY(hipMemcpyAsync(t.hpin.p, d_rows, nk * (sizeof(int64_t) + sizeof(float)), hipMemcpyDeviceToHost, s));
    RMU_HIP_TRY(hipStreamSynchronize(s));
    memcpy(out_rows, t.hpin.p, nk * sizeof(int64_t));
    if (out_scores) memcpy(out_scores, t.hpin.p + nk * sizeof(int64_t), nk * sizeof(float));
    t.finished(s, true);
    return RMU_OK;
}

// rrf_fuse.hip (rmu_hybrid_search; prototypes in rmu_common.h): the calling thread's stream, the dense member's list left on the device on it, and
// the end-of-call bookkeeping of the thread's workspaces
int rmu_thread_stream_(hipStream_t user, hipStream_t* s) {
    const int rc = g_tls.ensure_stream(user);
    if (rc) return rmu_fail(rc, "cannot create the calling thread's stream");
    *s = user ? user : g_tls.stream;
    return RMU_OK;
}
void rmu_thread_finished_(hipStream_t s, bool drained) { g_tls.finished(s, drained); }
int rmu_index_search_mmr_enqueue_(rmu_index_t* idx, const float* q, bool q_dev, int64_t nq, int fetch_k, int k, double lambda_mult, int64_t expect_rows,
                                  hipStream_t s, const char* who, std::shared_lock<std::shared_mutex>& lk, const int64_t** d_rows) {
    int64_t* rows = nullptr;
    const int rc = search_mmr_enqueue(idx, q, q_dev, nq, fetch_k, k, lambda_mult, 0, expect_rows, s, who, lk, &rows);
    *d_rows = rows;
    return rc;
}

extern "C" int rmu_index_search_mmr(rmu_index_t* idx, const float* q, int64_t nq, int fetch_k, int k, double lambda_mult, int64_t row_base,
                                    int64_t* out_rows, float* out_scores) {
    RMU_ENTRY();
    if (!idx || !q || !out_rows) return rmu_fail(RMU_E_INVALID, "rmu_index_search_mmr: null pointer");
    if (nq < 1 || fetch_k < 1 || fetch_k > 64 || k < 1 || k > fetch_k)
        return rmu_fail(RMU_E_INVALID, "rmu_index_search_mmr: nq >= 1, fetch_k in [1, 64], k in [1, fetch_k]");
    if (lambda_mult < 0.0) return rmu_fail(RMU_E_INVALID, "rmu_index_search_mmr: lambda_mult must be >= 0");
    Tls& t = g_tls;
    int rc = t.ensure_stream();
    if (rc) return rmu_fail(rc, "rmu_index_search_mmr: stream");
    return search_mmr_on(idx, q, false, nq, fetch_k, k, lambda_mult, row_base, out_rows, out_scores, t.stream, "rmu_index_search_mmr");
}

// bert.hip (rmu_bert_search_mmr): the same behind an encoder forward -- DEVICE queries on the encoder's stream
extern "C" int rmu_index_search_mmr_dev_(rmu_index_t* idx, const float* q_dev, int64_t nq, int fetch_k, int k, double lambda_mult, int64_t row_base,
                                         int64_t* out_rows, float* out_scores, void* hip_stream) {
    RMU_ENTRY();
    if (!idx || !q_dev || !out_rows || !hip_stream) return rmu_fail(RMU_E_INVALID, "rmu_bert_search_mmr: null pointer");
    if (nq < 1 || fetch_k < 1 || fetch_k > 64 || k < 1 || k > fetch_k)
        return rmu_fail(RMU_E_INVALID, "rmu_bert_search_mmr: nq >= 1, fetch_k in [1, 64], k in [1, fetch_k]");
    if (idx->dim != 384) return rmu_fail(RMU_E_INVALID, "rmu_bert_search_mmr: the index must hold 384-d rows (the encoder's width; a wide index never does)");
    Tls& t = g_tls;
    int rc = t.ensure_stream((hipStream_t)hip_stream);
    if (rc) return rmu_fail(rc, "rmu_bert_search_mmr: stream");
    return search_mmr_on(idx, q_dev, true, nq, fetch_k, k, lambda_mult, row_base, out_rows, out_scores, (hipStream_t)hip_stream, "rmu_bert_search_mmr");
}

// ------------------------------------------------------------------------------------------------
// persistence
// ------------------------------------------------------------------------------------------------
struct RmuFileHeader {
    char magic[8];          // "RMUIDX01"
    int32_t dim, dpad, metric, reserved;
    int64_t n, n_live;
    float xnorm_max;
    char pad[64 - 8 - 16 - 16 - 4];
};
static_assert(sizeof(RmuFileHeader) == 64, "header");

extern "C" int rmu_index_save(rmu_index_t* idx, const char* path) {
    RMU_ENTRY();
    if (!idx || !path) return rmu_fail(RMU_E_INVALID, "rmu_index_save: null argument");
    int rc = g_tls.ensure_stream();
    if (rc) return rmu_fail(rc, "rmu_index_save: stream");
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    FILE* f = fopen(path, "wb");
    if (!f) return rmu_fail(RMU_E_INVALID, std::string("rmu_index_save: cannot open ") + path);
    RmuFileHeader h{};
    memcpy(h.magic, "RMUIDX01", 8);
    h.dim = idx->dim; h.dpad = idx->dpad; h.metric = idx->metric; h.n = idx->n; h.n_live = idx->n_live; h.xnorm_max = idx->xnorm_max;
    bool ok = fwrite(&h, sizeof(h), 1, f) == 1;
    if (idx->n) ok = ok && fwrite(idx->alive.data(), 1, (size_t)idx->n, f) == (size_t)idx->n;
    const size_t rowb = (size_t)idx->dpad * sizeof(float);
    const int64_t chunk = 65536;                       // rows per staging copy (<= 192 MiB)
    std::vector<char> host(ok ? (size_t)std::min<int64_t>(chunk, std::max<int64_t>(idx->n, 1)) * rowb : 0);
    for (int64_t r0 = 0; ok && r0 < idx->n; r0 += chunk) {
        const int64_t nr = std::min<int64_t>(chunk, idx->n - r0);
        if (hipMemcpyAsync(host.data(), (const char*)idx->x + r0 * rowb, (size_t)nr * rowb, hipMemcpyDeviceToHost, g_tls.stream) != hipSuccess ||
            hipStreamSynchronize(g_tls.stream) != hipSuccess) {
            fclose(f);
            return rmu_fail(RMU_E_HIP, "rmu_index_save: device read");
        }
        ok = fwrite(host.data(), rowb, (size_t)nr, f) == (size_t)nr;
    }
    ok = (fclose(f) == 0) && ok;
    return ok ? RMU_OK : rmu_fail(RMU_E_INVALID, std::string("rmu_index_save: write failed: ") + path);
}

extern "C" int rmu_index_load(rmu_index_t** out, const char* path) {
    RMU_ENTRY();
    if (!out || !path) return rmu_fail(RMU_E_INVALID, "rmu_index_load: null argument");
    FILE* f = fopen(path, "rb");
    if (!f) return rmu_fail(RMU_E_INVALID, std::string("rmu_index_load: cannot open ") + path);
    RmuFileHeader h{};
    if (fread(&h, sizeof(h), 1, f) != 1 || memcmp(h.magic, "RMUIDX01", 8) != 0 || h.n < 0 || h.dim < 1 || h.dim > RMU_MAX_DIM_WIDE ||
        h.dpad != pad_dim_metric(h.dim, h.metric)) {
        fclose(f);
        return rmu_fail(RMU_E_INVALID, std::string("rmu_index_load: not an RMUIDX01 file: ") + path);
    }
    rmu_index_t* idx = nullptr;
    int rc = rmu_index_create(&idx, h.dim, h.metric, h.n > 0 ? h.n : 4096);
    if (rc) { fclose(f); return rc; }
    idx->alive.assign((size_t)h.n, 1);
    bool ok = h.n == 0 || fread(idx->alive.data(), 1, (size_t)h.n, f) == (size_t)h.n;
    const size_t rowb = (size_t)h.dpad * sizeof(float);
    const int64_t chunk = 65536;
    std::vector<char> host(ok ? (size_t)std::min<int64_t>(chunk, std::max<int64_t>(h.n, 1)) * rowb : 0);
    hipStream_t s = g_tls.stream;
    for (int64_t r0 = 0; ok && r0 < h.n; r0 += chunk) {
        const int64_t nr = std::min<int64_t>(chunk, h.n - r0);
        ok = fread(host.data(), rowb, (size_t)nr, f) == (size_t)nr;
        if (ok && hipMemcpyAsync((char*)idx->x + r0 * rowb, host.data(), (size_t)nr * rowb, hipMemcpyHostToDevice, s) != hipSuccess) ok = false;
        if (ok) ok = build_image(idx, r0, nr, s) == RMU_OK;
        if (ok && hipStreamSynchronize(s) != hipSuccess) ok = false;
        if (ok) fold_image_stats(idx);
    }
    fclose(f);
    if (!ok) { rmu_index_free(idx); return rmu_fail(RMU_E_INVALID, std::string("rmu_index_load: truncated or unreadable: ") + path); }
    idx->n = h.n; idx->n_live = h.n_live;
    if (h.xnorm_max > idx->xnorm_max) idx->xnorm_max = h.xnorm_max;
    *out = idx;
    return RMU_OK;
}

// ------------------------------------------------------------------------------------------------
// search
// ------------------------------------------------------------------------------------------------
static const int64_t kMaxQueriesPerLaunch = 8192;
static const int kScreenKp = 32;     // K': candidates the screening pass keeps per query (k <= 24)
// (round 5) 24 < k <= 32: K' = 40 -- the same eight spare candidates behind the k-th for the sufficiency test; the slots hold RMU_KS_CAP = 48
// (round 6) 32 < k <= 104 (BASELINE config 5's dense top-100): K' = k + max(8, k / 5), at most 120 -- the sufficiency test needs the K'-th approximate
// score 2 EPS below the k-th, and the order statistics crowd together as k grows (16..20 spare candidates at k = 100; 8 sufficed at k <= 32)
static const int kScreenMaxK = 104;
static inline int screen_kp(int k) {
    if (k <= 24) return kScreenKp;
    if (k <= 32) return 40;
    const int kp = k + (k / 5 > 8 ? k / 5 : 8);
    return kp < RMU_KS_CAP_DEEP - 8 ? kp : RMU_KS_CAP_DEEP - 8;
}

static u64* g_dbg = nullptr;         // RMU_SCAN_EXP=7: cycle / event counters of the scan kernels (diagnostics only)
static constexpr int kDbgWords = 17;   // (the kernels' counters: ScanLaunch::dbg)
static u64* dbg_buffer() {
#ifndef RMU_DEBUG_KERNELS
    return nullptr;          // the counter instantiations exist only in a --debug-kernels build
#endif
    static std::once_flag once;
    std::call_once(once, [] {
        if (rmu_env("RMU_SCAN_EXP") && atoi(rmu_env("RMU_SCAN_EXP")) == 7) (void)hipMalloc((void**)&g_dbg, kDbgWords * sizeof(u64));
    });
    return g_dbg;
}
static void dbg_dump(const char* what, int64_t rows, hipStream_t s) {
    u64 h[kDbgWords];
    (void)hipStreamSynchronize(s);
    (void)hipMemcpy(h, g_dbg, sizeof(h), hipMemcpyDeviceToHost);
    fprintf(stderr, "[rmu dbg %s: %lld rows] slow_tiles=%llu compactions=%llu appends=%llu wave_tiles=%llu spill_tiles=%llu clk_slow=%llu clk_bar=%llu clk_all=%llu clk_vmwait=%llu seg=%llu/%llu/%llu/%llu/%llu/%llu/%llu clk_pro=%llu\n",
            what, (long long)rows, h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8], h[9], h[10], h[11], h[12], h[13], h[14], h[15], h[16]);
    (void)hipMemset(g_dbg, 0, sizeof(h));
}

// row ranges of the threshold ladder over n rows (see the comment in screen_enqueue)
// first range of the ladder for batches of <= 128 queries (one query tile).  tools/ladder_sweep.py, 10M rows, same box, step ms at
// (ratio : first) 8:256 / 8:2048 / 8:16384 / 16:16384 / 32:16384 -- B = 1: 1.302 / 1.277 / 1.269 / 1.303 / 1.275; B = 32: 1.414 / 1.380 /
// 1.649 / 2.027 / 1.823; B = 128: 1.551 / 1.485 / 1.788 / 2.276 / 2.004 (profiles/r05_ladder_sweep.txt): one launch + merge less pays,
// a colder start does not.  Full batches keep 256 (1.25M rows x 1024: 1.245 ms at 256, 1.372 at 2048, 1.794 at 16384).
static constexpr int LADDER_FIRST_SMALL = 2048;
static std::vector<int64_t> ladder_bounds(int64_t n, int64_t nb, int opt_ratio = 0, int opt_first = 0) {
    // (per-index options RMU_OPT_LADDER_RATIO / _FIRST, then the defaults; a ratio of 1: a single cold launch)
    const int lvl_min = opt_first ? opt_first : (nb <= 128 ? LADDER_FIRST_SMALL : 256);
    // ratio 3 for full batches; small batches (one query tile, HBM-bound: 7.68 GB image per batch) have few appends to
    // save and pay for every launch gap and merge, so they climb faster
    // (round 4: from 4 096 rows up -- was 262 144.  A single COLD launch over 200k rows x 1024 queries takes 1.74 ms, twice what the ladder
    // needs for 1M rows: every score that beats a still-empty threshold is appended.  With the ladder: 200k 0.45 ms, 20k 0.27, 8k 0.29.)
    static const int64_t ladder_min = rmu_env("RMU_SCREEN_LADDER_MIN") ? atoll(rmu_env("RMU_SCREEN_LADDER_MIN")) : 4096;
    auto build = [&](int ratio) {
        std::vector<int64_t> b{n};
        if (ratio > 1 && n >= ladder_min) {
            int64_t c = n / ratio / 32 * 32;
            for (; c >= 65536 && b.size() < 24; c = c / ratio / 32 * 32) b.insert(b.begin(), c);
            // below 64k rows a range is a handful of tiles per workgroup and its appends cost next to nothing: ratio 8, down
            // to a first range so small (<= lvl_min rows) that its cold start -- every score is appended -- does not matter
            for (c = b.front() / 8 / 32 * 32; c >= lvl_min && b.size() < 24; c = c / 8 / 32 * 32) b.insert(b.begin(), c);
        }
        return b;
    };
    if (opt_ratio) return build(opt_ratio);
    if (nb <= 128) return build(8);
    // (round 6, second session) Full batches over a corpus below ~6M rows: a ladder level costs 40-60 us whatever its range (launch, query
    // fragments, emit, merge) while a seeded level's appends are cheap -- the ratio with the FEWEST levels wins there (ties: the smaller ratio).
    // tools/ladder_sweep.py, same box, step ms at ratio 3 / 4 / 8: 1M x 1024 0.970 / 1.004 / 0.949, x 512 0.632 / 0.643 / 0.604, x 256 0.434 / 0.445 / 0.402;
    // 1.25M x 1024 1.169 / 1.144 / 1.161, x 512 0.762 / 0.727 / 0.729, x 256 0.530 / 0.488 / 0.495; 2.5M x 1024 at 3 / 5: 1.97 / 1.92, x 256 0.699 / 0.670;
    // 4.5M x 1024 at 3 / 6: 3.30 / 3.25, x 256 1.092 / 1.022.  (Those sweeps predate band seeding and the spill path.)
    // 10M x 1024 with band and spill on (profiles/screen_refresh.md 5; one process, the ratios in turn): ratio 3 6.372 / 6.362 / 6.348 / 6.359
    // (mean 6.360, spread 0.024), ratio 4 6.304 / 6.376 / 6.358 (6.346), ratio 6 6.324 / 6.371 / 6.379 (6.358), ratio 8 6.359 / 6.383 / 6.382
    // (6.375): no ratio beats 3 by twice the spread of its own legs, with one level fewer or not, and the ratio stays 3.
    std::vector<int64_t> best = build(3);
    if (n < 6000000)
        for (int r : {4, 5, 6, 8}) {
            std::vector<int64_t> b = build(r);
            if (b.size() < best.size()) best = std::move(b);
        }
    return best;
}

// RMU_SCREEN_NOFILTER: ScanLaunch::share_thr bit 1 (timing ablation); RMU_NO_SHARED_THR: bit 0 off -- launches publish their thresholds, none
// reads them (debugging aid).  Each is read here and nowhere else.
static int nofilter_env() { static const int nofilter = rmu_env("RMU_SCREEN_NOFILTER") != nullptr ? 2 : 0; return nofilter; }
static int share_env() { static const int share = rmu_env("RMU_NO_SHARED_THR") ? 0 : 1; return share; }

// ---- the slot walk both threshold ladders share (screen_enqueue, search_block_deep).  One partial buffer holds, in slots of `part_keys`
// keys: [range 0's parts][merged 0 .. 0][range 1's parts][merged 0 .. 1][range 2's parts] ... -- a level's merge reads ONE contiguous run, the
// running top (absent at level 0) and behind it the level's own parts, and writes the slot behind that run, which heads the next level's.
static int ladder_slots(const std::vector<ScanLaunch>& lv) {
    int slots = (int)lv.size() - 1;
    for (const ScanLaunch& S : lv) slots += S.parts;
    return slots;
}
// A level's launch writes its part lists at `parts`; its merge reads `n_lists` lists from `merge_in` on and writes `merged`: the next
// level's running top, or `final_keys` behind the last level.
struct LadderLevel { u64* parts; const u64* merge_in; int n_lists; u64* merged; };
// level l of nl, whose launch writes `parts` lists; *slot (0 before level 0) walks the buffer `base`: call once per level, in order
static LadderLevel ladder_level(u64* base, size_t part_keys, int* slot, int l, int nl, int parts, u64* final_keys) {
    u64* const in = base + (size_t)*slot * part_keys;     // the running top (l > 0), else this range's first part
    const int n_lists = parts + (l > 0 ? 1 : 0);
    *slot += n_lists;                                     // -> the slot behind the run
    return {in + (size_t)(n_lists - parts) * part_keys, in, n_lists, l + 1 < nl ? in + (size_t)n_lists * part_keys : final_keys};
}

// Enqueue the screening ladder for `nb` device queries (fp32, [nb, 384]): on return (stream order) t.ckeys holds the best
// K' approximate candidates per query, sorted.  No host synchronisation.  scan_ms_events: record per-launch events.
// Threshold ladder: the corpus is scanned in row ranges of geometrically growing size (256 rows, x8 up to 64k, then x3);
// after each range its candidates are merged with the running top-K' and the K'-th best seeds the shared per-query
// thresholds of the next launch.  A cold launch appends K' ln(rows/K') candidates per query and CHUNK, a seeded one only
// K' (ratio - 1) per query in total, and every append stalls a whole workgroup for ~1-3k cycles: this cut
// the filter overhead of the 10M x 1024 scan from 5.2 to ~1.5 ms.  `k` (the caller's k) below `kp`: the merges also seed the lower edge of
// the sufficiency band (see `band` below), about a third of those appends.
static int screen_enqueue(rmu_index* idx, Tls& t, const float* qdev, int64_t nb, hipStream_t s, bool timed, int* n_launches,
                          ScanLaunch* last_geom, int k, int kp = kScreenKp, u32* zero_word = nullptr /* one more word the query conversion zeroes (the re-run count) */) {
    const int share = share_env();
    const std::vector<int64_t> bounds = ladder_bounds(idx->n, nb, idx->ladder_ratio, idx->ladder_first);
    const int nl = (int)bounds.size();
    std::vector<ScanLaunch> lv((size_t)nl);
    size_t pwords = 0;                                   // sibling-pacing progress words: [s_chunks][4] per paced launch
    size_t gcand_bytes = 0;                              // global candidate slots (reused by every launch of the ladder)
    for (int l = 0; l < nl; ++l) {
        ScanLaunch& S = lv[(size_t)l];
        S = ScanLaunch{};
        S.x = (const float*)idx->split; S.row0 = l ? bounds[(size_t)l - 1] : 0; S.n_rows = bounds[(size_t)l] - S.row0;
        S.dpad = 384; S.nq = (int)nb; S.k = kp;       // (the image's geometry; an L2 index keeps its fp32 rows 768 floats apart)
        S.nrm = idx->nrm;
        if (rmu_screen_plan(&S) != RMU_OK) return rmu_fail(RMU_E_INVALID, "rmu_index_search: screening geometry");
        if (S.pace) pwords += (size_t)S.s_chunks * 4;
        gcand_bytes = std::max(gcand_bytes, (size_t)S.parts * (size_t)nb * (kp > RMU_KS_CAP - 8 ? RMU_KS_CAP_DEEP : RMU_KS_CAP) * sizeof(u64));
    }
    const size_t part_keys = (size_t)nb * kp;
    const size_t gwords = (size_t)((nb + 255) / 256 * 256 + 64);
    const size_t gbytes = (gwords + pwords) * sizeof(u32);    // one memset zeroes thresholds and progress words
    if (gcand_bytes && t.gcand.ensure(gcand_bytes)) return rmu_fail(RMU_E_OOM, "rmu_index_search: screening candidate slots");
    // Spill path (RMU_OPT_SCREEN_SPILL, scan_screen.hip "Spill path"): the SEEDED launches of the 8-wave kernels leave the accumulators of
    // passing lanes in per-wave lists and rmu_sift_launch takes the place of their merge.  The cold first launch, the 4-wave kernels and the
    // filter's debugging modes (RMU_NO_SHARED_THR, RMU_SCREEN_NOFILTER) go the old way; switched off, the ladder is enqueued as it always was.
    // kSpillCap records per list.  Debug counters of the headline (10M x 1024, band on, profiles/screen_spill.md): the fullest levels, 13 504
    // and 108 032 rows, leave 69 384 / 68 465 passing scores in 1 952 / 2 048 lists -- 36 per list, and a record holds at least one of them;
    // the four large levels leave 10 per list.  256 is seven times that mean (a Poisson count of mean 36 passes 256 with a probability
    // below 1e-100; the scores of a list are those of 32 queries that each contribute one or two) and holds two tiles in which EVERY lane
    // passes for both groups (2 x 128 records).  A list that still overflows costs nothing but time: its wave goes on through slow_path.
    static constexpr int kSpillCap = 256;
    const int spill_cap = idx->spill_cap > 0 ? idx->spill_cap : kSpillCap;
    size_t spill_lists = 0;
    if (idx->screen_spill && share && !nofilter_env())
        for (int l = 1; l < nl; ++l)
            if (lv[(size_t)l].wq == 8) spill_lists = std::max(spill_lists, (size_t)lv[(size_t)l].s_chunks * (size_t)lv[(size_t)l].nqt * 8);
    if (spill_lists && (t.spill.ensure(spill_lists * (size_t)spill_cap * RMU_SPILL_REC) || t.spill_cnt.ensure(spill_lists * sizeof(u32))))
        return rmu_fail(RMU_E_OOM, "rmu_index_search: screening spill lists");
    if (t.partial.ensure((size_t)ladder_slots(lv) * part_keys * sizeof(u64)) || t.qsplit.ensure((size_t)nb * RMU_IMG_ROW_BYTES) ||
        t.gthr.ensure(gbytes) || t.ckeys.ensure(part_keys * sizeof(u64)) || t.eps.ensure((size_t)nb * sizeof(float)) || t.ensure_events(2 * nl))
        return rmu_fail(RMU_E_OOM, "rmu_index_search: screening workspace");
    const int sflags = share | nofilter_env();
    // (an L2 index holds its queries as (2q, 1): the image is fp16(64 q) all the same)
    // (round 6) the conversion's first workgroup also zeroes the ladder's thresholds + pacing words and the caller's word: was two memsets
    // Band seeding (scan_screen.hip header): a seeded launch needs only the rows that can reach the caller's top-k or decide its sufficiency
    // test -- s~ above s~[k-1] - 2 EPS(q), about rank 11-12 of K' = 32 at k = 10 -- so the merges publish that edge beside the K'-th key, and a
    // level appends about a third of the K' (ratio - 1) candidates per query.  EPS(q) is computed by the query conversion (no launch of its own).
    // k = K' (rmu_index_screen_candidates) or RMU_OPT_SCREEN_BAND = 0: the K'-th key alone, as before.
    const bool band = idx->screen_band && k < kp && nl > 1;
    const bool l2q = idx->metric == RMU_METRIC_L2SQ;
    int rc = rmu_split_launch(qdev, t.qsplit.p, nb, s, idx->dpad, l2q ? 32.0f : 64.0f, (u32*)t.gthr.p,
                              (int)(gbytes / sizeof(u32)), zero_word, zero_word ? 1 : 0, band ? (float*)t.eps.p : nullptr, idx->xnorm_max, idx->dx_max,
                              l2q ? 1 : 0);
    if (rc) return rmu_fail(rc, "rmu_index_search: query conversion");
    int slot = 0;
    u32* prog_next = (u32*)t.gthr.p + gwords;
    for (int l = 0; l < nl; ++l) {
        ScanLaunch& S = lv[(size_t)l];
        const LadderLevel lvl = ladder_level((u64*)t.partial.p, part_keys, &slot, l, nl, S.parts, (u64*)t.ckeys.p);
        u32* const seed = l + 1 < nl ? (u32*)t.gthr.p : nullptr;       // merge + seed the next launch's thresholds in one launch
        S.prog = nullptr;
        if (S.pace) { S.prog = prog_next; prog_next += (size_t)S.s_chunks * 4; }
        S.partial = lvl.parts;
        // (round 6) the FIRST launch is cold -- one tile per chunk, every row a candidate -- and its slots leave unsorted (share_thr bit 2; its merge
        // below is told): sorting 32 keys for each of a workgroup's 256 queries was ~25 us of a launch that scans 2 000 rows.  RMU_EMIT_RAW=0: never.
        static const int emit_raw = (rmu_env("RMU_EMIT_RAW") && atoi(rmu_env("RMU_EMIT_RAW")) == 0) ? 0 : 4;
        const int raw = l == 0 ? emit_raw : 0;
        S.gthr = (u32*)t.gthr.p; S.share_thr = sflags | raw; S.dbg = g_dbg; S.q = (const float*)t.qsplit.p;
        S.gcand = (u64*)t.gcand.p;
        const bool spill = spill_lists != 0 && l > 0 && S.wq == 8;
        if (spill) { S.spill = (char*)t.spill.p; S.spill_cnt = (u32*)t.spill_cnt.p; S.spill_cap = spill_cap; }
        if (spill && idx->screen_refresh) S.share_thr |= 8;     // RMU_OPT_SCREEN_REFRESH = 1: no wave of the launch drops its refresh (scan_screen.hip "Refresh")
        if (timed) RMU_HIP_TRY(hipEventRecord(t.lev[(size_t)(2 * l)], s));
        rc = rmu_screen_launch(&S, s);
        if (rc) return rmu_fail(rc, "rmu_index_search: screening launch");
        if (timed) RMU_HIP_TRY(hipEventRecord(t.lev[(size_t)(2 * l + 1)], s));
        if (g_dbg) dbg_dump("screen range", S.n_rows, s);
        if (spill)       // the running top-K' (the head of the merge's run) + this launch's spill lists (+ the part lists of waves that fell back)
            rc = rmu_sift_launch(&S, lvl.merge_in, nb, kp, lvl.merged, seed, s, k, band ? (const float*)t.eps.p : nullptr);
        else
            rc = rmu_merge_to_keys_band_launch(lvl.merge_in, lvl.n_lists, nb, kp, lvl.merged, seed, s, raw ? 1 : 0, k,
                                               band ? (const float*)t.eps.p : nullptr);
        if (rc) return rmu_fail(rc, "rmu_index_search: screening merge / threshold seeding");
    }
    *n_launches = nl;
    if (last_geom) *last_geom = lv.back();
    return RMU_OK;
}

static bool screen_applies(const rmu_index* idx, int64_t nb, int k) {
    // (read once: the per-index switch is rmu_index_set_option(RMU_OPT_SCREEN_MIN_NQ))
    static const bool env_set = rmu_env("RMU_SCREEN_MIN_NQ") != nullptr;
    static const int env_min_nq = env_set ? atoi(rmu_env("RMU_SCREEN_MIN_NQ")) : 1;
    const bool min_nq_set = env_set || idx->screen_min_nq > 0;
    const int64_t screen_min_nq = idx->screen_min_nq > 0 ? idx->screen_min_nq : env_min_nq;
    // small batches are HBM-bound either way: the screen reads half the bytes (768 vs 1536 B per row) but pays for the
    // ladder's launches and merges per batch, which only pays off on a large enough corpus
    // (deep k: the alternative is the exact 128-deep ladder at ~0.3 of the HBM roof -- the screen pays from the size that ladder starts at)
    const bool screen_pays = nb >= 128 || idx->n >= 3000000 || (nb > 64 && idx->n >= 1000000) || min_nq_set || (k > 32 && idx->n >= 262144);
    const bool geom = idx->dim == 384 && (idx->metric == RMU_METRIC_L2SQ ? idx->nrm != nullptr : idx->dpad == 384);
    if (idx->wide_scan) return false;   // RMU_OPT_WIDE_SCAN: every search is the exact scan, through scan_wide_kernel
    return idx->split && idx->screen_enabled && geom &&
           nb >= screen_min_nq && screen_pays && k <= kScreenMaxK && idx->n > 0 && idx->xnorm_max > 0.f &&
           idx->xnorm_max < 500.f;   // fp16(64*x) must not overflow
}

// deep k (the 128-deep candidate geometry) over a large corpus takes the exact scan as a threshold ladder (see rmu_index_search)
static bool deep_applies(const rmu_index* idx, int k) {
    static const bool off = rmu_env("RMU_DEEP") && atoi(rmu_env("RMU_DEEP")) == 0;
    return !off && k > 32 && idx->n >= 262144;
}
static std::vector<int64_t> deep_bounds(int64_t n) {
    static const int first = rmu_env("RMU_DEEP_FIRST") ? atoi(rmu_env("RMU_DEEP_FIRST")) : 8192;
    static const int ratio = rmu_env("RMU_DEEP_RATIO") ? atoi(rmu_env("RMU_DEEP_RATIO")) : 4;
    std::vector<int64_t> b{n};
    for (int64_t c = n / ratio / 128 * 128; c >= first && b.size() < 8; c = c / ratio / 128 * 128) b.insert(b.begin(), c);
    return b;
}

// ---- what rmu_index_search and rmu_index_search_subset do alike for a block of nb queries (`who` opens the error text).  The subset
// search promises the unfiltered search's bits: both are given the SAME prepared queries by the one function below. -----------------
// bytes of the shared per-query thresholds of n queries: padded to whole 128-query tiles, zero = no bound yet
static size_t gthr_bytes(int64_t n) { return (size_t)((n + 127) / 128 * 128 + 64) * sizeof(u32); }

// queries -> device, padded to dpad, normalised for COSINE, augmented for L2SQ (t.qn = |q|^2 per query; dpad > dim by construction there:
// such queries are always copied).  *qdev = the prepared queries: t.q, or qsrc itself where nothing has to change
static int prepare_queries(const rmu_index* idx, Tls& t, const float* qsrc, int64_t nb, bool q_dev, hipStream_t s, const float** qdev, const char* who) {
    const int dpad = idx->dpad, dim = idx->dim;
    *qdev = qsrc;
    const bool need_copy = !q_dev || dpad != dim || idx->metric == RMU_METRIC_COSINE;
    if (!need_copy) return RMU_OK;
    if (t.q.ensure((size_t)nb * dpad * sizeof(float))) return rmu_fail(RMU_E_OOM, std::string(who) + ": q workspace");
    if (dpad != dim) RMU_HIP_TRY(hipMemsetAsync(t.q.p, 0, (size_t)nb * dpad * sizeof(float), s));
    RMU_HIP_TRY(hipMemcpy2DAsync(t.q.p, (size_t)dpad * sizeof(float), qsrc, (size_t)dim * sizeof(float),
                             (size_t)dim * sizeof(float), (size_t)nb,
                             q_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    if (idx->metric == RMU_METRIC_COSINE) {
        hipLaunchKernelGGL(k_row_norm, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, s, (float*)t.q.p, dpad, nb, 1,
                           (float*)nullptr);
        RMU_HIP_TRY(hipGetLastError());
    }
    if (idx->metric == RMU_METRIC_L2SQ) {
        if (t.qn.ensure((size_t)nb * sizeof(float))) return rmu_fail(RMU_E_OOM, std::string(who) + ": |q|^2 workspace");
        hipLaunchKernelGGL(k_l2_aug_queries, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, s, (float*)t.q.p, dpad, dim, nb,
                           (float*)t.qn.p);
        RMU_HIP_TRY(hipGetLastError());
    }
    *qdev = (const float*)t.q.p;
    return RMU_OK;
}

// host outputs: the block's results are staged in this thread's device buffers (*d_s, *d_r are redirected there) ...
static int stage_outputs(Tls& t, int64_t nb, int k, bool out_dev, float** d_s, int64_t** d_r, const char* who) {
    if (out_dev) return RMU_OK;
    if (t.out_s.ensure((size_t)nb * k * sizeof(float)) || t.out_r.ensure((size_t)nb * k * sizeof(int64_t)))
        return rmu_fail(RMU_E_OOM, std::string(who) + ": output workspace");
    *d_s = (float*)t.out_s.p;
    *d_r = (int64_t*)t.out_r.p;
    return RMU_OK;
}
// ... and copied to the caller's arrays behind the block's work
static int copy_outputs(float* out_scores, int64_t* out_rows, int64_t q0, int64_t nb, int k, bool out_dev, const float* d_s, const int64_t* d_r,
                        hipStream_t s) {
    if (out_dev) return RMU_OK;
    RMU_HIP_TRY(hipMemcpyAsync(out_scores + q0 * k, d_s, (size_t)nb * k * sizeof(float), hipMemcpyDeviceToHost, s));
    RMU_HIP_TRY(hipMemcpyAsync(out_rows + q0 * k, d_r, (size_t)nb * k * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    return RMU_OK;
}

static float elapsed_ms(hipEvent_t a, hipEvent_t b) { float ms = 0.f; return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.f; }

// ---- one block of at most kMaxQueriesPerLaunch queries, as the path that answers it sees it (rmu_index_search fills it in) ----------
struct SearchBlock {
    rmu_index* idx; Tls& t; hipStream_t s;
    const float* qdev; int64_t nb; int k; int64_t row_base;    // the prepared queries (prepare_queries)
    float* d_s; int64_t* d_r;                                   // where the block's results go on the device (stage_outputs)
    bool timed, l2;
    // ... and what the path hands back
    float scan_ms = 0.f;        // scan time it has measured itself (the screening ladder's per-launch events)
    bool exact_timed = false;   // t.ev[2] .. t.ev[3] bracket its scans: read by rmu_index_search behind the block's drain
};

// the three paths that answer a block (defined behind rmu_index_search, which chooses among them)
static int search_block_screened(SearchBlock& b), search_block_deep(SearchBlock& b), search_block_exact(SearchBlock& b);

extern "C" int rmu_index_search(rmu_index_t* idx, const float* q, int64_t nq, int k, unsigned flags, int64_t row_base,
                                float* out_scores, int64_t* out_rows, uint64_t hip_stream) {
    RMU_ENTRY();
    if (!idx || !q || !out_scores || !out_rows) return rmu_fail(RMU_E_INVALID, "rmu_index_search: null pointer");
    if (nq < 1) return rmu_fail(RMU_E_INVALID, "rmu_index_search: nq must be >= 1");
    if (k < 1 || k > RMU_MAX_K) return rmu_fail(RMU_E_INVALID, "rmu_index_search: k must be in [1, 112]");
    Tls& t = g_tls;
    int rc = t.ensure_stream((hipStream_t)hip_stream);
    if (rc) return rmu_fail(rc, "rmu_index_search: stream");
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : t.stream;
    const bool q_dev = flags & RMU_F_Q_DEVICE, out_dev = flags & RMU_F_OUT_DEVICE;
    const bool timed = t.timing && !hip_stream;
    (void)dbg_buffer();

    std::shared_lock<std::shared_mutex> lk(idx->mu);
    const bool l2 = idx->metric == RMU_METRIC_L2SQ;     // dpad > dim by construction: queries are always copied and augmented
    t.scan_ms = -1.f; t.search_ms = -1.f; t.passes = 0; t.screened = 0;
    float scan_total = 0.f;
    bool any_screened = false;
    int rerun_total = 0;
    if (timed) RMU_HIP_TRY(hipEventRecord(t.ev[0], s));
    if (t.ensure_hflag()) return rmu_fail(RMU_E_OOM, "rmu_index_search: pinned flag");

    for (int64_t q0 = 0; q0 < nq; q0 += kMaxQueriesPerLaunch) {
        const int64_t nb = (nq - q0) < kMaxQueriesPerLaunch ? (nq - q0) : kMaxQueriesPerLaunch;
        const float* qdev;
        if ((rc = prepare_queries(idx, t, q + q0 * idx->dim, nb, q_dev, s, &qdev, "rmu_index_search"))) return rc;
        float* d_s = out_scores + q0 * k; int64_t* d_r = out_rows + q0 * k;
        if ((rc = stage_outputs(t, nb, k, out_dev, &d_s, &d_r, "rmu_index_search"))) return rc;
        SearchBlock b{idx, t, s, qdev, nb, k, row_base, d_s, d_r, timed, l2};
        const bool screened = screen_applies(idx, nb, k);
        if (screened) rc = search_block_screened(b);
        else if (deep_applies(idx, k)) rc = search_block_deep(b);
        else rc = search_block_exact(b);
        if (rc) return rc;
        scan_total += b.scan_ms;
        if ((rc = copy_outputs(out_scores, out_rows, q0, nb, k, out_dev, d_s, d_r, s))) return rc;
        // workspace is reused by the next query block (and host outputs must land): drain per block.  With a caller stream,
        // device outputs and a single block nothing here waits: the work is merely ordered on that stream.
        const bool drained = !hip_stream || q0 + nb < nq || !out_dev;
        if (drained) RMU_HIP_TRY(hipStreamSynchronize(s));
        else mark_reader(idx, s);
        t.finished(s, drained);
        if (screened) {   // the count of re-run queries is unknown while a caller's stream still runs: reported as 0 then
            any_screened = true;
            if (drained) rerun_total += *t.hflag;
        }
        if (b.exact_timed) {
            RMU_HIP_TRY(hipEventSynchronize(t.ev[3]));
            scan_total += elapsed_ms(t.ev[2], t.ev[3]);
        }
    }
    t.screened = any_screened ? (rerun_total ? -rerun_total : 1) : 0;
    if (timed) {
        RMU_HIP_TRY(hipEventRecord(t.ev[1], s));
        RMU_HIP_TRY(hipEventSynchronize(t.ev[1]));
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, t.ev[0], t.ev[1]) == hipSuccess) t.search_ms = ms;
        t.scan_ms = scan_total;
    }
    return RMU_OK;
}

// ---- the exact fp32 fused scan + merge of `nqq` device queries: plan first, then run.  ALL workspace of a block is sized before anything
// that uses it is enqueued (a grow-only buffer must not be re-allocated under work already in flight), and no RmuDevBuf::ensure may run between
// taking a buffer's pointer and the launch that uses it -- so a path plans every launch it may need, sizes t.partial / t.gthr for the largest
// (exact_partial_bytes, gthr_bytes), and only then runs them; run_exact takes the pointers itself.  `cond` (optional) makes both launches
// conditional on the device-side count of flagged queries; `scatter` redirects result row i to batch row scatter[i]. ---------------------
static int plan_exact(const SearchBlock& b, const float* qd, int64_t nqq, const RmuCond* cond, ScanLaunch* L) {
    *L = ScanLaunch{};
    L->x = b.idx->x; L->n_rows = b.idx->n; L->dpad = b.idx->dpad; L->q = qd; L->nq = (int)nqq; L->k = b.k; L->dbg = g_dbg;
    L->wide = b.idx->wide_scan ? 1 : 0;     // (a dpad above 768 is routed to the wide kernel by the planner itself)
    if (cond) L->cond = *cond;
    const int rc = rmu_scan_plan(L);
    return rc ? rmu_fail(rc, "rmu_index_search: no scan geometry for this (dim, k)") : RMU_OK;
}
// bytes of a planned launch's partial lists (a launch that was never planned: 0)
static size_t exact_partial_bytes(const ScanLaunch& L) { return (size_t)L.parts * L.nq * L.k * sizeof(u64); }

// zero_gthr_bytes: bytes of the shared thresholds to zero in front of the launch (0: an earlier launch of a mutually exclusive
// group already did -- only ONE launch of such a group ever runs, and a launch that does not run touches nothing)
static int run_exact(SearchBlock& b, ScanLaunch& L, float* os, int64_t* orr, const int64_t* scatter, bool time_it, size_t zero_gthr_bytes) {
    Tls& t = b.t; hipStream_t s = b.s;
    const bool has_cond = L.cond.p != nullptr;
    L.partial = (u64*)t.partial.p;
    L.gthr = (u32*)t.gthr.p;
    L.share_thr = share_env();
    if (zero_gthr_bytes) RMU_HIP_TRY(hipMemsetAsync(t.gthr.p, 0, zero_gthr_bytes, s));
    int rc;
    if (b.idx->n > 0) {
        if (time_it) RMU_HIP_TRY(hipEventRecord(t.ev[2], s));
        rc = rmu_scan_launch(&L, s);
        if (rc) return rmu_fail(rc, std::string("rmu_index_search: scan launch: ") + hipGetErrorString(hipGetLastError()));
        if (time_it) { RMU_HIP_TRY(hipEventRecord(t.ev[3], s)); b.exact_timed = true; }
        if (!has_cond) t.note_geometry(L, 1);
    } else {
        RMU_HIP_TRY(hipMemsetAsync(L.partial, 0, exact_partial_bytes(L), s));
    }
    rc = rmu_merge_final_launch(L.partial, L.parts, L.nq, L.k, b.row_base, b.l2 ? 1 : 0, b.l2 ? (const float*)t.qn.p : nullptr, os, orr,
                                scatter, has_cond ? &L.cond : nullptr, s);
    if (rc) return rmu_fail(rc, "rmu_index_search: merge launch");
    if (g_dbg && !has_cond) dbg_dump("exact", b.idx->n, s);
    return RMU_OK;
}

// ---- screened path: fp16 scan proposes K' = 32 candidates, exact fp32 re-score decides ------------------------------------------------
// Flagged queries -> exact scan, decided ON THE DEVICE: three mutually exclusive conditional launches
//   1..32 flagged: the 32-query HBM-bound geometry; 33..nb/8: a batch of nb/8; more: the whole batch.
// With nothing flagged (the normal case) each costs one empty grid (~2 us); no host round trip either way, so
// the whole search is asynchronous on the stream it was given.
// (round 5) Every dependent launch of a search costs ~4.4 us of kernel boundary on this part, run or not, and a batch of <= 32
// queries already IS the 32-query geometry: one class there -- "anything flagged: the exact scan of the whole batch" -- without
// the gather (3 stream operations behind the re-score instead of 7); the classes of a larger batch share ONE threshold memset.
static int search_block_screened(SearchBlock& b) {
    rmu_index* idx = b.idx; Tls& t = b.t; hipStream_t s = b.s;
    const float* qdev = b.qdev; const int64_t nb = b.nb; const int k = b.k, dpad = idx->dpad;
    float* d_s = b.d_s; int64_t* d_r = b.d_r;
    int rc;
    const bool one_class = nb <= 32;
    const int small_n = (int)(nb < 32 ? nb : 32), mid_n = one_class ? 0 : (int)(nb / 8);
    const int gather_n = mid_n > small_n ? mid_n : small_n;
    const int lim_small = one_class ? 0 : (mid_n > small_n ? small_n : mid_n);    // no mid launch: the small one covers 1..nb/8
    if (t.flag.ensure(2 * sizeof(int)) || t.fb_i.ensure((size_t)nb * sizeof(int64_t)) ||
        t.fbq.ensure((size_t)gather_n * dpad * sizeof(float)))
        return rmu_fail(RMU_E_OOM, "rmu_index_search: re-run workspace");
    const int* cnt = (const int*)t.flag.p;
    const RmuCond c1{cnt, 1, lim_small, 1}, c2{cnt, small_n + 1, mid_n, 1}, c3{cnt, (lim_small > 0 || mid_n > small_n ? mid_n : 0) + 1, 0x7fffffff, 0};
    ScanLaunch L1{}, L2{}, L3{};
    if (lim_small > 0 && (rc = plan_exact(b, (const float*)t.fbq.p, small_n, &c1, &L1))) return rc;
    if (mid_n > small_n && (rc = plan_exact(b, (const float*)t.fbq.p, mid_n, &c2, &L2))) return rc;
    if ((rc = plan_exact(b, qdev, nb, &c3, &L3))) return rc;
    const size_t need_partial = std::max({exact_partial_bytes(L1), exact_partial_bytes(L2), exact_partial_bytes(L3)});
    const size_t need_gthr = gthr_bytes(nb);           // (L3's: the gathered launches are planned for fewer queries)
    if (t.partial.ensure(need_partial) || t.gthr.ensure(need_gthr)) return rmu_fail(RMU_E_OOM, "rmu_index_search: re-run partials");
    int nl = 0;
    ScanLaunch lastg{};
    if ((rc = screen_enqueue(idx, t, qdev, nb, s, b.timed, &nl, &lastg, k, screen_kp(k), (u32*)t.flag.p))) return rc;    // (flag[0] = 0 by the query conversion)
    // |s~ - s_fp32| <= EPS(q) from the measured image errors (derivation in scan_screen.hip); queries failing the
    // sufficiency test are appended to the list fb_i (count in flag[0])
    rc = rmu_rescore_launch((const u64*)t.ckeys.p, screen_kp(k), idx->x, qdev, nb, k, idx->xnorm_max, idx->dx_max, b.row_base, d_s, d_r,
                            (int*)t.flag.p, (int64_t*)t.fb_i.p, nullptr, s, dpad, b.l2 ? (const float*)t.qn.p : nullptr);
    if (rc) return rmu_fail(rc, "rmu_index_search: re-score launch");
    t.note_geometry(lastg, nl);
    // gather (batches above 32 queries) + the re-runs' threshold zeroing + the count to the host, one launch (see the kernel)
    const int g_n = (lim_small > 0 || mid_n > small_n) ? gather_n : 0;
    hipLaunchKernelGGL(k_gather_flagged, dim3((unsigned)(g_n > 0 ? g_n : 1)), dim3(128), 0, s, qdev, dpad, (const int64_t*)t.fb_i.p, cnt,
                       (float*)t.fbq.p, g_n, (u32*)t.gthr.p, (int)(need_gthr / sizeof(u32)), t.hflag_dev);
    RMU_HIP_TRY(hipGetLastError());
    // (zero_gthr_bytes = 0: the thresholds of the mutually exclusive re-run launches were zeroed by the launch above)
    if (lim_small > 0 && (rc = run_exact(b, L1, d_s, d_r, (const int64_t*)t.fb_i.p, false, 0))) return rc;
    if (mid_n > small_n && (rc = run_exact(b, L2, d_s, d_r, (const int64_t*)t.fb_i.p, false, 0))) return rc;
    if ((rc = run_exact(b, L3, d_s, d_r, nullptr, false, 0))) return rc;
    if (b.timed)
        for (int l = 0; l < nl; ++l) {
            RMU_HIP_TRY(hipEventSynchronize(t.lev[(size_t)(2 * l + 1)]));
            b.scan_ms += elapsed_ms(t.lev[(size_t)(2 * l)], t.lev[(size_t)(2 * l + 1)]);
        }
    return RMU_OK;
}

// ---- deep k (32 < k <= 112) over a large corpus (BASELINE config 5's dense top-100): the 128-deep scan is slow COLD --
// k ln(rows / k) appends per query and chunk, each stalling a barrier-coupled workgroup -- not per byte.  So the
// threshold ladder of the screening path, with exact arithmetic: the corpus is scanned in row ranges of growing size
// (~8k rows, then x4), after each range the candidates are merged with the running top-k (keys) and its k-th best
// seeds the shared per-query thresholds of the next launch; the last merge writes the results.  Every launch is
// the exact fp32 scan, every bound is a real k-th best: results are those of the single launch, bit for bit.
static int search_block_deep(SearchBlock& b) {
    rmu_index* idx = b.idx; Tls& t = b.t; hipStream_t s = b.s;
    const int64_t nb = b.nb; const int k = b.k, dpad = idx->dpad;
    int rc;
    const std::vector<int64_t> bounds = deep_bounds(idx->n);
    const int nl = (int)bounds.size();
    std::vector<ScanLaunch> lv((size_t)nl);
    for (int l = 0; l < nl; ++l) {
        ScanLaunch& S = lv[(size_t)l];
        S = ScanLaunch{};
        S.row0 = l ? bounds[(size_t)l - 1] : 0;
        S.x = idx->x + S.row0 * dpad; S.n_rows = bounds[(size_t)l] - S.row0; S.dpad = dpad; S.q = b.qdev; S.nq = (int)nb; S.k = k; S.dbg = g_dbg;
        S.wide = idx->wide_scan ? 1 : 0;
        if ((rc = rmu_scan_plan(&S))) return rmu_fail(rc, "rmu_index_search: no scan geometry for this (dim, k)");
    }
    const size_t part_keys = (size_t)nb * k;
    const size_t gthr_need = gthr_bytes(nb);
    if (t.partial.ensure((size_t)ladder_slots(lv) * part_keys * sizeof(u64)) || t.gthr.ensure(gthr_need))
        return rmu_fail(RMU_E_OOM, "rmu_index_search: ladder workspace");
    RMU_HIP_TRY(hipMemsetAsync(t.gthr.p, 0, gthr_need, s));
    int slot = 0;
    if (b.timed) RMU_HIP_TRY(hipEventRecord(t.ev[2], s));
    for (int l = 0; l < nl; ++l) {
        ScanLaunch& S = lv[(size_t)l];
        const LadderLevel lvl = ladder_level((u64*)t.partial.p, part_keys, &slot, l, nl, S.parts, nullptr /* the last merge writes results, not keys */);
        S.partial = lvl.parts; S.gthr = (u32*)t.gthr.p; S.share_thr = share_env();
        rc = rmu_scan_launch(&S, s);
        if (rc) return rmu_fail(rc, std::string("rmu_index_search: scan launch: ") + hipGetErrorString(hipGetLastError()));
        if (l + 1 < nl)
            rc = rmu_merge_to_keys_launch(lvl.merge_in, lvl.n_lists, nb, k, lvl.merged, (u32*)t.gthr.p, s);
        else
            rc = rmu_merge_final_launch(lvl.merge_in, lvl.n_lists, nb, k, b.row_base, b.l2 ? 1 : 0, b.l2 ? (const float*)t.qn.p : nullptr,
                                        b.d_s, b.d_r, nullptr, nullptr, s);
        if (rc) return rmu_fail(rc, "rmu_index_search: ladder merge");
    }
    if (b.timed) { RMU_HIP_TRY(hipEventRecord(t.ev[3], s)); b.exact_timed = true; }
    t.note_geometry(lv.back(), nl);
    return RMU_OK;
}

// ---- everything else: one exact scan of the whole block ---------------------------------------------------------------------------------
static int search_block_exact(SearchBlock& b) {
    Tls& t = b.t;
    ScanLaunch L{};
    int rc;
    if ((rc = plan_exact(b, b.qdev, b.nb, nullptr, &L))) return rc;
    if (t.partial.ensure(exact_partial_bytes(L)) || t.gthr.ensure(gthr_bytes(b.nb))) return rmu_fail(RMU_E_OOM, "rmu_index_search: partial workspace");
    return run_exact(b, L, b.d_s, b.d_r, nullptr, b.timed, gthr_bytes(b.nb));
}

// Exact top-k over the rows one ascending list names (include/rmu.h): the gathered scan of scan_subset.hip, whose keys carry list
// positions, the ordinary final merge, then positions -> row ids.  The query preparation is rmu_index_search's (same padded, normalised,
// augmented queries: the scores have the same bits).
extern "C" int rmu_index_search_subset(rmu_index_t* idx, const float* q, int64_t nq, int k, unsigned flags, int64_t row_base,
                                       const int64_t* rows, int64_t n_sub, float* out_scores, int64_t* out_rows, uint64_t hip_stream) {
    RMU_ENTRY();
    if (!idx || !q || !out_scores || !out_rows) return rmu_fail(RMU_E_INVALID, "rmu_index_search_subset: null pointer");
    if (nq < 1) return rmu_fail(RMU_E_INVALID, "rmu_index_search_subset: nq must be >= 1");
    if (k < 1 || k > RMU_MAX_K) return rmu_fail(RMU_E_INVALID, "rmu_index_search_subset: k must be in [1, 112]");
    if (n_sub < 0 || (n_sub > 0 && !rows)) return rmu_fail(RMU_E_INVALID, "rmu_index_search_subset: rows / n_sub");
    Tls& t = g_tls;
    int rc = t.ensure_stream((hipStream_t)hip_stream);
    if (rc) return rmu_fail(rc, "rmu_index_search_subset: stream");
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : t.stream;
    const bool q_dev = flags & RMU_F_Q_DEVICE, out_dev = flags & RMU_F_OUT_DEVICE, rows_dev = flags & RMU_F_ROWS_DEVICE;

    std::shared_lock<std::shared_mutex> lk(idx->mu);
    const int dpad = idx->dpad, dim = idx->dim;
    const bool l2 = idx->metric == RMU_METRIC_L2SQ;
    if (dpad > RMU_MAX_DIM)
        return rmu_fail(RMU_E_INVALID, "rmu_index_search_subset: the index holds rows wider than 768 dimensions (RMU_MAX_DIM): the filtered search "
                                   "does not serve a wide index yet");
    if (!rows_dev) {            // a host list is checked before anything is enqueued; a device list is the caller's contract
        int64_t prev = -1;
        for (int64_t i = 0; i < n_sub; ++i) {
            const int64_t r = rows[i];
            if (r <= prev || r >= idx->n)
                return rmu_fail(RMU_E_INVALID, "rmu_index_search_subset: rows must be strictly ascending ids in [0, n): entry " + std::to_string(i));
            prev = r;
        }
    }
    if (n_sub >= 0xFFFFFFFFll || idx->n >= 0xFFFFFFFFll) return rmu_fail(RMU_E_INVALID, "rmu_index_search_subset: row ids must fit 32 bits");
    const int64_t n_eff = idx->n > 0 ? n_sub : 0;       // (an empty index: every id of a device list is absent)
    t.scan_ms = -1.f; t.search_ms = -1.f; t.passes = 0; t.screened = 0;
    if (n_eff > 0) {
        if (t.sub_ids.ensure((size_t)rmu_subset_ids_len(n_eff) * sizeof(u32))) return rmu_fail(RMU_E_OOM, "rmu_index_search_subset: id workspace");
        const int64_t* drows = rows;
        if (!rows_dev) {
            if (t.sub_rows.ensure((size_t)n_eff * sizeof(int64_t))) return rmu_fail(RMU_E_OOM, "rmu_index_search_subset: list workspace");
            RMU_HIP_TRY(hipMemcpyAsync(t.sub_rows.p, rows, (size_t)n_eff * sizeof(int64_t), hipMemcpyHostToDevice, s));
            drows = (const int64_t*)t.sub_rows.p;
        }
        if ((rc = rmu_subset_narrow_launch(drows, n_eff, idx->n, (u32*)t.sub_ids.p, s))) return rmu_fail(rc, "rmu_index_search_subset: list conversion");
    }

    for (int64_t q0 = 0; q0 < nq; q0 += kMaxQueriesPerLaunch) {
        const int64_t nb = (nq - q0) < kMaxQueriesPerLaunch ? (nq - q0) : kMaxQueriesPerLaunch;
        const float* qdev;
        if ((rc = prepare_queries(idx, t, q + q0 * dim, nb, q_dev, s, &qdev, "rmu_index_search_subset"))) return rc;
        float* d_s = out_scores + q0 * k; int64_t* d_r = out_rows + q0 * k;
        if ((rc = stage_outputs(t, nb, k, out_dev, &d_s, &d_r, "rmu_index_search_subset"))) return rc;
        int parts = 1;
        if (n_eff > 0) {
            SubsetLaunch L{};
            L.x = idx->x; L.n_rows = idx->n; L.dpad = dpad; L.ids = (const u32*)t.sub_ids.p; L.n_sub = n_eff; L.q = qdev; L.nq = (int)nb; L.k = k;
            if ((rc = rmu_subset_plan(&L))) return rmu_fail(rc, "rmu_index_search_subset: no scan geometry for this (dim, k)");
            if (t.partial.ensure((size_t)L.parts * nb * k * sizeof(u64)) || t.gthr.ensure(gthr_bytes(nb)))
                return rmu_fail(RMU_E_OOM, "rmu_index_search_subset: partial workspace");
            L.partial = (u64*)t.partial.p;
            L.gthr = (u32*)t.gthr.p;
            RMU_HIP_TRY(hipMemsetAsync(t.gthr.p, 0, gthr_bytes(nb), s));
            rc = rmu_subset_launch(&L, s);
            if (rc) return rmu_fail(rc, std::string("rmu_index_search_subset: scan launch: ") + hipGetErrorString(hipGetLastError()));
            t.note_geometry(L, 1);
            parts = L.parts;
        } else {               // nothing to scan: one all-empty partial, every slot comes out (-inf | +inf, -1)
            if (t.partial.ensure((size_t)nb * k * sizeof(u64))) return rmu_fail(RMU_E_OOM, "rmu_index_search_subset: partial workspace");
            RMU_HIP_TRY(hipMemsetAsync(t.partial.p, 0, (size_t)nb * k * sizeof(u64), s));
        }
        rc = rmu_merge_final_launch((const u64*)t.partial.p, parts, nb, k, 0, l2 ? 1 : 0, l2 ? (const float*)t.qn.p : nullptr, d_s, d_r, nullptr,
                                    nullptr, s);
        if (rc) return rmu_fail(rc, "rmu_index_search_subset: merge launch");
        if (n_eff > 0 && (rc = rmu_subset_map_launch(d_r, (const u32*)t.sub_ids.p, nb * k, row_base, s)))
            return rmu_fail(rc, "rmu_index_search_subset: row id launch");
        if ((rc = copy_outputs(out_scores, out_rows, q0, nb, k, out_dev, d_s, d_r, s))) return rc;
        // as rmu_index_search: drain per block unless this is the only block of a caller stream with device outputs.  A host list was
        // copied from pageable memory the caller may reuse: that call drains as well.
        const bool drained = !hip_stream || q0 + nb < nq || !out_dev || !rows_dev;
        if (drained) RMU_HIP_TRY(hipStreamSynchronize(s));
        else mark_reader(idx, s);
        t.finished(s, drained);
    }
    return RMU_OK;
}

// One list per group of adjacent queries, every group in one call (include/rmu.h): the lists a query uses are narrowed end to end, the
// planner (rmu_groups_plan) writes one descriptor per workgroup, at most two scan launches (one per geometry class) fill a ZEROED
// [P, nq, k] partial buffer, then the ordinary final merge and positions -> row ids through each query's own list.  The work table, the
// used lists and the per-query offsets travel through this thread's pinned buffer in ONE copy, so the call always drains its stream.
extern "C" int rmu_index_search_groups(rmu_index_t* idx, const float* q, int64_t nq, int k, unsigned flags, int64_t row_base,
                                       const int64_t* rows, const int64_t* list_ptr, int n_lists, const int32_t* q_list,
                                       float* out_scores, int64_t* out_rows, uint64_t hip_stream) {
    RMU_ENTRY();
    // everything that needs neither the index nor the device comes first
    if (nq < 1 || nq > kMaxQueriesPerLaunch) return rmu_fail(RMU_E_INVALID, "rmu_index_search_groups: nq must be in [1, 8192]");
    if (k < 1 || k > RMU_MAX_K) return rmu_fail(RMU_E_INVALID, "rmu_index_search_groups: k must be in [1, 112]");
    if (n_lists < 1) return rmu_fail(RMU_E_INVALID, "rmu_index_search_groups: n_lists must be >= 1");
    if (!q || !out_scores || !out_rows || !list_ptr || !q_list) return rmu_fail(RMU_E_INVALID, "rmu_index_search_groups: null pointer");
    if (list_ptr[0] != 0) return rmu_fail(RMU_E_INVALID, "rmu_index_search_groups: list_ptr[0] must be 0");
    for (int g = 0; g < n_lists; ++g)
        if (list_ptr[g + 1] < list_ptr[g]) return rmu_fail(RMU_E_INVALID, "rmu_index_search_groups: list_ptr must be non-decreasing: entry " + std::to_string(g + 1));
    const int64_t n_all = list_ptr[n_lists];
    if (n_all >= 0xFFFFFFFFll) return rmu_fail(RMU_E_INVALID, "rmu_index_search_groups: the lists together must hold fewer than 2^32 rows");
    if (n_all > 0 && !rows) return rmu_fail(RMU_E_INVALID, "rmu_index_search_groups: rows is null");
    for (int64_t i = 0; i < nq; ++i)
        if (q_list[i] < 0 || q_list[i] >= n_lists || (i > 0 && q_list[i] < q_list[i - 1]))
            return rmu_fail(RMU_E_INVALID, "rmu_index_search_groups: q_list must be non-decreasing list numbers in [0, n_lists): entry " + std::to_string(i));
    if (!idx) return rmu_fail(RMU_E_INVALID, "rmu_index_search_groups: null index");
    Tls& t = g_tls;
    int rc = t.ensure_stream((hipStream_t)hip_stream);
    if (rc) return rmu_fail(rc, "rmu_index_search_groups: stream");
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : t.stream;
    const bool q_dev = flags & RMU_F_Q_DEVICE, out_dev = flags & RMU_F_OUT_DEVICE, rows_dev = flags & RMU_F_ROWS_DEVICE;

    std::shared_lock<std::shared_mutex> lk(idx->mu);
    const int dpad = idx->dpad;
    const bool l2 = idx->metric == RMU_METRIC_L2SQ;
    if (dpad > RMU_MAX_DIM)
        return rmu_fail(RMU_E_INVALID, "rmu_index_search_groups: the index holds rows wider than 768 dimensions (RMU_MAX_DIM): the filtered search "
                                   "does not serve a wide index yet");
    if (idx->n >= 0xFFFFFFFFll) return rmu_fail(RMU_E_INVALID, "rmu_index_search_groups: row ids must fit 32 bits");
    if (!rows_dev) {            // host lists are checked before anything is enqueued; device lists are the caller's contract
        for (int g = 0; g < n_lists; ++g) {
            int64_t prev = -1;
            for (int64_t i = list_ptr[g]; i < list_ptr[g + 1]; ++i) {
                const int64_t r = rows[i];
                if (r <= prev || r >= idx->n)
                    return rmu_fail(RMU_E_INVALID, "rmu_index_search_groups: every list must hold strictly ascending ids in [0, n): list " +
                                               std::to_string(g) + ", entry " + std::to_string(i - list_ptr[g]));
                prev = r;
            }
        }
    }
    GroupsPlan P;
    if ((rc = rmu_groups_plan(dpad, k, (int)nq, list_ptr, q_list, &P))) return rmu_fail(rc, "rmu_index_search_groups: no scan geometry for this (dim, k)");
    const bool scan = idx->n > 0 && !P.lists.empty();       // (an empty index: every id of a device list is absent)
    const int parts = scan ? P.parts : 1;
    t.scan_ms = -1.f; t.search_ms = -1.f; t.passes = 0; t.screened = 0;

    const float* qdev;
    if ((rc = prepare_queries(idx, t, q, nq, q_dev, s, &qdev, "rmu_index_search_groups"))) return rc;
    float* d_s = out_scores; int64_t* d_r = out_rows;
    if ((rc = stage_outputs(t, nq, k, out_dev, &d_s, &d_r, "rmu_index_search_groups"))) return rc;
    const size_t partial_bytes = (size_t)parts * nq * k * sizeof(u64), gthr_len = (size_t)(nq + 128) * sizeof(u32);
    if (t.partial.ensure(partial_bytes) || t.gthr.ensure(gthr_len)) return rmu_fail(RMU_E_OOM, "rmu_index_search_groups: partial workspace");
    RMU_HIP_TRY(hipMemsetAsync(t.partial.p, 0, partial_bytes, s));     // a group's missing parts, and the queries of empty lists: empty
    if (scan) {
        // table: [descriptors of class 0][of class 1][used lists][per-query offsets], pinned -> device in one copy
        const size_t b_t0 = P.tab[0].size() * sizeof(GroupDesc), b_t1 = P.tab[1].size() * sizeof(GroupDesc);
        const size_t b_l = P.lists.size() * sizeof(GroupList), b_q = (size_t)nq * sizeof(u32), b_all = b_t0 + b_t1 + b_l + b_q;
        if (t.hpin.ensure(b_all) || t.gtab.ensure(b_all) || t.sub_ids.ensure((size_t)P.ids_total * sizeof(u32)))
            return rmu_fail(RMU_E_OOM, "rmu_index_search_groups: table / id workspace");
        if (b_t0) memcpy(t.hpin.p, P.tab[0].data(), b_t0);
        if (b_t1) memcpy(t.hpin.p + b_t0, P.tab[1].data(), b_t1);
        memcpy(t.hpin.p + b_t0 + b_t1, P.lists.data(), b_l);
        memcpy(t.hpin.p + b_t0 + b_t1 + b_l, P.q_off.data(), b_q);
        RMU_HIP_TRY(hipMemcpyAsync(t.gtab.p, t.hpin.p, b_all, hipMemcpyHostToDevice, s));
        const char* tab = (const char*)t.gtab.p;
        const int64_t* drows = rows;
        if (!rows_dev) {
            if (t.sub_rows.ensure((size_t)n_all * sizeof(int64_t))) return rmu_fail(RMU_E_OOM, "rmu_index_search_groups: list workspace");
            RMU_HIP_TRY(hipMemcpyAsync(t.sub_rows.p, rows, (size_t)n_all * sizeof(int64_t), hipMemcpyHostToDevice, s));
            drows = (const int64_t*)t.sub_rows.p;
        }
        if ((rc = rmu_groups_narrow_launch(drows, (const GroupList*)(tab + b_t0 + b_t1), (int)P.lists.size(), idx->n, (u32*)t.sub_ids.p, P.ids_total, s)))
            return rmu_fail(rc, "rmu_index_search_groups: list conversion");
        RMU_HIP_TRY(hipMemsetAsync(t.gthr.p, 0, gthr_len, s));
        if (t.timing) RMU_HIP_TRY(hipEventRecord(t.ev[2], s));         // rmu_set_timing: the scan launches between two events
        for (int cls = 0; cls < 2; ++cls) {
            if (P.tab[cls].empty()) continue;
            GroupsLaunch L{};
            L.x = idx->x; L.n_rows = idx->n; L.dpad = dpad; L.ids = (const u32*)t.sub_ids.p; L.q = qdev; L.nq = (int)nq; L.k = k;
            L.partial = (u64*)t.partial.p; L.gthr = (u32*)t.gthr.p;
            L.tab = (const GroupDesc*)(tab + (cls ? b_t0 : 0));
            L.wq = cls ? 4 : 1; L.kv = k <= 32 ? 0 : 1; L.grid = (int)P.tab[cls].size(); L.lds_bytes = P.lds_bytes[cls];
            rc = rmu_groups_launch(&L, s);
            if (rc) return rmu_fail(rc, std::string("rmu_index_search_groups: scan launch: ") + hipGetErrorString(hipGetLastError()));
            t.note_geometry(L, 1);
        }
        if (t.timing) RMU_HIP_TRY(hipEventRecord(t.ev[3], s));
    }
    rc = rmu_merge_final_launch((const u64*)t.partial.p, parts, nq, k, 0, l2 ? 1 : 0, l2 ? (const float*)t.qn.p : nullptr, d_s, d_r, nullptr,
                                nullptr, s);
    if (rc) return rmu_fail(rc, "rmu_index_search_groups: merge launch");
    if (scan) {
        const size_t q_off_at = (P.tab[0].size() + P.tab[1].size()) * sizeof(GroupDesc) + P.lists.size() * sizeof(GroupList);
        if ((rc = rmu_groups_map_launch(d_r, (const u32*)t.sub_ids.p, (const u32*)((const char*)t.gtab.p + q_off_at), nq * k, k, row_base, s)))
            return rmu_fail(rc, "rmu_index_search_groups: row id launch");
    }
    if ((rc = copy_outputs(out_scores, out_rows, 0, nq, k, out_dev, d_s, d_r, s))) return rc;
    RMU_HIP_TRY(hipStreamSynchronize(s));          // always: the table went through the thread's pinned buffer
    t.finished(s, true);
    if (t.timing && scan) t.scan_ms = elapsed_ms(t.ev[2], t.ev[3]);
    return RMU_OK;
}

// Grouped top-k behind rmu_index_search_distinct (columns.hip; prototype in rmu_common.h): per block of queries the distinct scan
// (scan_distinct.hip) fills [parts, nb, k] part lists, k_distinct_fold folds them into [nb, k] distinct keys behind them in the same
// workspace, and rmu_index_search's own finishing (rmu_merge_final_launch over ONE list) writes scores, row ids + row_base, the L2
// conversion and the padding.  The query preparation is rmu_index_search's (same padded, normalised, augmented queries: the scores have
// the same bits).  The caller holds the columns' shared lock for the codes: every block is drained before this returns.
int rmu_index_search_distinct_on_(rmu_index* idx, const int32_t* codes_dev, int64_t expect_rows, const float* q, int64_t nq, int k, unsigned flags,
                                  int64_t row_base, float* out_scores, int64_t* out_rows, hipStream_t user_stream) {
    const char* who = "rmu_index_search_distinct";
    Tls& t = g_tls;
    int rc = t.ensure_stream(user_stream);
    if (rc) return rmu_fail(rc, std::string(who) + ": stream");
    hipStream_t s = user_stream ? user_stream : t.stream;
    const bool q_dev = flags & RMU_F_Q_DEVICE, out_dev = flags & RMU_F_OUT_DEVICE;

    std::shared_lock<std::shared_mutex> lk(idx->mu);
    const int dpad = idx->dpad, dim = idx->dim;
    const bool l2 = idx->metric == RMU_METRIC_L2SQ;
    if (dpad > RMU_MAX_DIM)
        return rmu_fail(RMU_E_INVALID, std::string(who) + ": the index holds rows wider than 768 dimensions (RMU_MAX_DIM): the grouped search does "
                                                          "not serve a wide index");
    if (idx->n != expect_rows)
        return rmu_fail(RMU_E_INVALID, std::string(who) + ": the columns (" + std::to_string(expect_rows) + " rows) and the index (" +
                                           std::to_string(idx->n) + " rows) are out of step");
    if (idx->n >= 0xFFFFFFFFll) return rmu_fail(RMU_E_INVALID, std::string(who) + ": row ids must fit 32 bits");
    const bool scan = idx->n > 0 && idx->n_live > 0 && codes_dev != nullptr;
    t.scan_ms = -1.f; t.search_ms = -1.f; t.passes = 0; t.screened = 0; t.fold_ms = -1.f; t.fold_parts = 0;

    for (int64_t q0 = 0; q0 < nq; q0 += kMaxQueriesPerLaunch) {
        const int64_t nb = (nq - q0) < kMaxQueriesPerLaunch ? (nq - q0) : kMaxQueriesPerLaunch;
        const float* qdev;
        if ((rc = prepare_queries(idx, t, q + q0 * dim, nb, q_dev, s, &qdev, who))) return rc;
        float* d_s = out_scores + q0 * k; int64_t* d_r = out_rows + q0 * k;
        if ((rc = stage_outputs(t, nb, k, out_dev, &d_s, &d_r, who))) return rc;
        const size_t list_keys = (size_t)nb * k;
        const u64* folded;
        if (scan) {
            DistinctLaunch L{};
            L.x = idx->x; L.n_rows = idx->n; L.dpad = dpad; L.codes = codes_dev; L.q = qdev; L.nq = (int)nb; L.k = k;
            if ((rc = rmu_distinct_plan(&L))) return rmu_fail(rc, std::string(who) + ": no scan geometry for this (dim, k)");
            if (t.partial.ensure(((size_t)L.parts + 1) * list_keys * sizeof(u64))) return rmu_fail(RMU_E_OOM, std::string(who) + ": partial workspace");
            L.partial = (u64*)t.partial.p;
            u64* out_keys = L.partial + (size_t)L.parts * list_keys;
            if (t.timing) RMU_HIP_TRY(hipEventRecord(t.ev[2], s));        // rmu_set_timing: the scan between two events, the fold between two more
            rc = rmu_distinct_launch(&L, s);
            if (rc) return rmu_fail(rc, std::string(who) + ": scan launch: " + hipGetErrorString(hipGetLastError()));
            if (t.timing) { RMU_HIP_TRY(hipEventRecord(t.ev[3], s)); RMU_HIP_TRY(hipEventRecord(t.ev[4], s)); }
            if ((rc = rmu_distinct_fold_launch(L.partial, L.parts, nb, k, codes_dev, out_keys, s))) return rmu_fail(rc, std::string(who) + ": fold launch");
            if (t.timing) RMU_HIP_TRY(hipEventRecord(t.ev[5], s));
            t.note_geometry(L, 1);
            t.fold_parts = L.parts;
            folded = out_keys;
        } else {               // nothing to scan: one all-empty list, every slot comes out (-inf | +inf, -1)
            if (t.partial.ensure(list_keys * sizeof(u64))) return rmu_fail(RMU_E_OOM, std::string(who) + ": partial workspace");
            RMU_HIP_TRY(hipMemsetAsync(t.partial.p, 0, list_keys * sizeof(u64), s));
            folded = (const u64*)t.partial.p;
        }
        rc = rmu_merge_final_launch(folded, 1, nb, k, row_base, l2 ? 1 : 0, l2 ? (const float*)t.qn.p : nullptr, d_s, d_r, nullptr, nullptr, s);
        if (rc) return rmu_fail(rc, std::string(who) + ": merge launch");
        if ((rc = copy_outputs(out_scores, out_rows, q0, nb, k, out_dev, d_s, d_r, s))) return rc;
        RMU_HIP_TRY(hipStreamSynchronize(s));          // always: the caller's lock on the codes ends with this call
        t.finished(s, true);
        if (t.timing && scan) { t.scan_ms = elapsed_ms(t.ev[2], t.ev[3]); t.fold_ms = elapsed_ms(t.ev[4], t.ev[5]); }
    }
    return RMU_OK;
}
// (probe hook, not in rmu.h; tools/distinct_probe.py) the calling thread's last grouped search under rmu_set_timing: the fold's kernel time
// (< 0 = not taken) and the part lists it folded -- of the last block of queries
extern "C" int rmu_last_distinct_(float* fold_ms, int* parts) {
    if (fold_ms) *fold_ms = g_tls.fold_ms;
    if (parts) *parts = g_tls.fold_parts;
    return RMU_OK;
}

// Test hook (not a product entry point): the screening pass's candidate set for each query -- approximate scores s~,
// row ids, and the per-query error bound EPS(q) the sufficiency test uses -- so the bound |s~ - s_fp32| <= EPS can be
// checked ON THE HARDWARE against fp32 scores computed independently (tests/test_search_gpu.py).
extern "C" int rmu_index_screen_candidates(rmu_index_t* idx, const float* q_host, int64_t nq, float* out_approx, int64_t* out_rows,
                                           float* out_exact, float* out_eps) {
    RMU_ENTRY();
    if (!idx || !q_host || !out_approx || !out_rows || !out_exact || !out_eps) return rmu_fail(RMU_E_INVALID, "rmu_index_screen_candidates: null pointer");
    if (nq < 1 || nq > kMaxQueriesPerLaunch) return rmu_fail(RMU_E_INVALID, "rmu_index_screen_candidates: 1 <= nq <= 8192");
    Tls& t = g_tls;
    int rc = t.ensure_stream();
    if (rc) return rmu_fail(rc, "rmu_index_screen_candidates: stream");
    hipStream_t s = t.stream;
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    if (!idx->split || idx->dim != 384 || idx->n <= 0) return rmu_fail(RMU_E_INVALID, "rmu_index_screen_candidates: index has no screening image");
    if (idx->metric == RMU_METRIC_L2SQ) return rmu_fail(RMU_E_INVALID, "rmu_index_screen_candidates: inner-product / cosine indexes only");
    const int kp = kScreenKp;
    if (t.flag.ensure((size_t)(nq + 1) * sizeof(int)) || t.fb_i.ensure((size_t)nq * sizeof(int64_t)) ||
        t.out_s.ensure((size_t)nq * kp * sizeof(float)) || t.out_r.ensure((size_t)nq * kp * sizeof(int64_t)) || t.nrm.ensure((size_t)nq * sizeof(float)))
        return rmu_fail(RMU_E_OOM, "rmu_index_screen_candidates: workspace");
    const float* qdev;
    if ((rc = prepare_queries(idx, t, q_host, nq, false, s, &qdev, "rmu_index_screen_candidates"))) return rc;
    RMU_HIP_TRY(hipMemsetAsync(t.flag.p, 0, sizeof(int), s));
    int nl = 0;
    rc = screen_enqueue(idx, t, qdev, nq, s, false, &nl, nullptr, kp /* k = K': no band -- the true approximate top-K' */);
    if (rc) return rc;
    // k = K': the re-score kernel writes the exact fp32 score of EVERY candidate (rank order) and EPS(q)
    rc = rmu_rescore_launch((const u64*)t.ckeys.p, kp, idx->x, qdev, nq, kp, idx->xnorm_max, idx->dx_max, 0, (float*)t.out_s.p,
                            (int64_t*)t.out_r.p, (int*)t.flag.p, (int64_t*)t.fb_i.p, (float*)t.nrm.p, s);
    if (rc) return rmu_fail(rc, "rmu_index_screen_candidates: re-score");
    std::vector<u64> keys((size_t)nq * kp);
    std::vector<float> ex((size_t)nq * kp);
    std::vector<int64_t> er((size_t)nq * kp);
    RMU_HIP_TRY(hipMemcpyAsync(keys.data(), t.ckeys.p, keys.size() * sizeof(u64), hipMemcpyDeviceToHost, s));
    RMU_HIP_TRY(hipMemcpyAsync(ex.data(), t.out_s.p, ex.size() * sizeof(float), hipMemcpyDeviceToHost, s));
    RMU_HIP_TRY(hipMemcpyAsync(er.data(), t.out_r.p, er.size() * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    RMU_HIP_TRY(hipMemcpyAsync(out_eps, t.nrm.p, (size_t)nq * sizeof(float), hipMemcpyDeviceToHost, s));
    RMU_HIP_TRY(hipStreamSynchronize(s));
    for (int64_t i = 0; i < nq; ++i)
        for (int c = 0; c < kp; ++c) {
            const u64 key = keys[(size_t)(i * kp + c)];
            out_approx[i * kp + c] = key ? rmu_key_score(key) : -INFINITY;
            out_rows[i * kp + c] = key ? (int64_t)rmu_key_row(key) : -1;
            // exact fp32 score of that same row: look it up in the re-scored (exact-rank-ordered) list
            float e = -INFINITY;
            for (int c2 = 0; c2 < kp && key; ++c2)
                if (er[(size_t)(i * kp + c2)] == (int64_t)rmu_key_row(key)) { e = ex[(size_t)(i * kp + c2)]; break; }
            out_exact[i * kp + c] = e;
        }
    return RMU_OK;
}

extern "C" int rmu_index_set_option(rmu_index_t* idx, int option, int64_t value) {
    if (!idx) return rmu_fail(RMU_E_INVALID, "rmu_index_set_option: null index");
    std::unique_lock<std::shared_mutex> lk(idx->mu);
    switch (option) {
        case RMU_OPT_SCREEN: idx->screen_enabled = value != 0; return RMU_OK;
        case RMU_OPT_SCREEN_MIN_NQ: idx->screen_min_nq = value > 0 ? value : 0; return RMU_OK;
        case RMU_OPT_LADDER_RATIO: idx->ladder_ratio = value > 0 && value <= 4096 ? (int)value : 0; return RMU_OK;
        case RMU_OPT_LADDER_FIRST: idx->ladder_first = value > 0 && value <= (1 << 30) ? (int)value : 0; return RMU_OK;
        case RMU_OPT_SCREEN_BAND: idx->screen_band = value != 0; return RMU_OK;
        case RMU_OPT_SCREEN_SPILL: idx->screen_spill = value != 0; return RMU_OK;
        case RMU_OPT_SCREEN_SPILL_CAP: idx->spill_cap = value > 0 && value <= 4096 ? (int)value : 0; return RMU_OK;
        case RMU_OPT_SCREEN_REFRESH: idx->screen_refresh = value != 0; return RMU_OK;
        case RMU_OPT_COMPACT_INPLACE: idx->compact_inplace = value != 0; return RMU_OK;
        case RMU_OPT_WIDE_SCAN:
            if (idx->metric == RMU_METRIC_L2SQ) return rmu_fail(RMU_E_INVALID, "rmu_index_set_option: RMU_OPT_WIDE_SCAN serves RMU_METRIC_IP / RMU_METRIC_COSINE indexes only");
            if (value != 0 && value != 1) return rmu_fail(RMU_E_INVALID, "rmu_index_set_option: RMU_OPT_WIDE_SCAN takes 0 or 1");
            idx->wide_scan = value == 1;
            return RMU_OK;
        default: return rmu_fail(RMU_E_INVALID, "rmu_index_set_option: unknown option");
    }
}
extern "C" int rmu_index_metric(rmu_index_t* idx, int* metric) {
    if (!idx || !metric) return rmu_fail(RMU_E_INVALID, "rmu_index_metric: null");
    *metric = idx->metric;
    return RMU_OK;
}

extern "C" int rmu_topk_merge(const float* scores, const int64_t* rows, int parts, int64_t nq, int k, unsigned flags,
                              float* out_scores, int64_t* out_rows, uint64_t hip_stream) {
    RMU_ENTRY();
    if (!scores || !rows || !out_scores || !out_rows) return rmu_fail(RMU_E_INVALID, "rmu_topk_merge: null pointer");
    if (parts < 1 || nq < 1 || k < 1 || k > 128) return rmu_fail(RMU_E_INVALID, "rmu_topk_merge: parts/nq >= 1, k in [1,128]");
    Tls& t = g_tls;
    int rc = t.ensure_stream((hipStream_t)hip_stream);
    if (rc) return rmu_fail(rc, "rmu_topk_merge: stream");
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : t.stream;
    const bool in_dev = flags & RMU_F_Q_DEVICE, out_dev = flags & RMU_F_OUT_DEVICE;
    const size_t cnt = (size_t)parts * nq * k;
    const float* ds = scores; const int64_t* dr = rows;
    if (!in_dev) {
        if (t.in_s.ensure(cnt * sizeof(float)) || t.in_r.ensure(cnt * sizeof(int64_t)))
            return rmu_fail(RMU_E_OOM, "rmu_topk_merge: input workspace");
        RMU_HIP_TRY(hipMemcpyAsync(t.in_s.p, scores, cnt * sizeof(float), hipMemcpyHostToDevice, s));
        RMU_HIP_TRY(hipMemcpyAsync(t.in_r.p, rows, cnt * sizeof(int64_t), hipMemcpyHostToDevice, s));
        ds = (const float*)t.in_s.p;
        dr = (const int64_t*)t.in_r.p;
    }
    float* os = out_scores; int64_t* orr = out_rows;
    if ((rc = stage_outputs(t, nq, k, out_dev, &os, &orr, "rmu_topk_merge"))) return rc;
    rc = rmu_merge_lists_launch(ds, dr, parts, nq * k, nq * k, nq, k, (flags & RMU_F_SMALLER_BETTER) ? 1 : 0, os, orr, s);
    if (rc) return rmu_fail(rc, "rmu_topk_merge: launch");
    if ((rc = copy_outputs(out_scores, out_rows, 0, nq, k, out_dev, os, orr, s))) return rc;
    const bool drained = !hip_stream || !out_dev || !in_dev;
    if (drained) RMU_HIP_TRY(hipStreamSynchronize(s));
    t.finished(s, drained);
    return RMU_OK;
}

// rrf_fuse.hip -- weighted reciprocal-rank fusion on the device, and the reference's whole retrieval step as ONE call (gfx950 only).
//
// Serves: EnsembleRetriever([bm25, dense_mmr], weights=[0.5, 0.5]).invoke -- what every chain of the reference calls (server/RAGHelper.py:497-503,
// RAGHelper_local.py:251-259): langchain's weighted_reciprocal_rank over the members' lists, documents identified by page_content.
//
// rmu_rrf_fuse restates ragmeup_amd/ensemble.py's weighted_reciprocal_rank over integer keys.  Per query, with the entries of the lists taken in
// CHAIN order (list 0 first, positions ascending):
//   rank(entry)  = 1 + the present (key >= 0) entries in front of it in its own list
//   score(key)   = the fp64 sum, in chain order and starting from 0.0, of weights[l] / (rank + c) over every entry that holds the key
//   output       = the distinct keys by score descending, equal scores in order of their first entries; each key is reported with the
//                  (list, position) of its first entry.
// The quotients are computed on the HOST (at most 448 doubles) and the kernel only adds them, in the order Python adds them: the scores have
// Python's bits, and the order needs no tolerance.
//
// Kernel (rrf_fuse_kernel): one workgroup per query, the <= 448 entries staged in LDS as (key, contribution).  An entry is FIRST iff no earlier
// entry holds its key; a first entry sums the later entries of its key; its output slot is the number of first entries with a larger score, or
// an equal score and an earlier place in the chain.  O(n^2) compares on broadcast LDS reads, no atomics, no sort network: deterministic.
//
// rmu_hybrid_search enqueues, on the calling thread's stream: the BM25 search (first half of bm25.hip's search), the dense search + MMR (first
// half of rmu_api.hip's search_mmr_on), the SAME kernel reading the two device-resident id lists through the key tables (key = table[id]: the
// members' ids become page_content classes) -- then one copy, one synchronisation.  Both members' shared locks are held until the stream is
// drained, as in their own searches.
#include <cmath>
#include <cstring>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <vector>

#include "../../include/rmu.h"
#include "rmu_common.h"
#include "rmu_host.h"
#include "rmu_internal.h"      // rmu_hybrid_check_ / rmu_hybrid_search_dev_: the prototypes bert.hip calls them by


namespace {

constexpr int kBlock = 256;
constexpr int kMaxEntries = RMU_RRF_MAX_LISTS * RMU_MAX_K;      // 448

struct RrfLaunch {
    const int64_t* ids[RMU_RRF_MAX_LISTS];     // list l of query q = ids[l] + q * len[l], len[l] <= depth entries; nullptr = an empty list
    const int64_t* table[RMU_RRF_MAX_LISTS];   // nullptr: the entries ARE keys; else key = table[id] for 0 <= id < table_len, absent otherwise
    int64_t table_len[RMU_RRF_MAX_LISTS];
    int len[RMU_RRF_MAX_LISTS];
    const double* contrib;                     // [lists, depth]: weights[l] / (rank + c) at [l, rank - 1]
    double* out_scores;                        // [nq, k_out]
    int64_t* out_keys;                         // [nq, k_out]: the key -- or, with `resolve`, the entry itself (the member's own id)
    int32_t* out_src;                          // [nq, k_out]: list * depth + position of the first entry -- or, with `resolve`, the list
    int lists, depth, k_out, resolve;
};

__global__ __launch_bounds__(kBlock) void rrf_fuse_kernel(RrfLaunch p) {
    __shared__ int64_t s_key[kMaxEntries];
    __shared__ double s_val[kMaxEntries];      // the entry's contribution (0 for an absent one)
    __shared__ double s_score[kMaxEntries];    // a first entry: its key's score (>= 0); every other entry: -1
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    const int depth = p.depth, n = p.lists * depth;

    // 1. stage the keys (static list indices: the launch descriptor stays in the kernel-argument segment)
#pragma unroll
    for (int l = 0; l < RMU_RRF_MAX_LISTS; ++l) {
        if (l >= p.lists) break;
        const int64_t* src = p.ids[l];
        const int64_t* tab = p.table[l];
        const int64_t tab_len = p.table_len[l];
        const int len = p.len[l];
        for (int pos = tid; pos < depth; pos += kBlock) {
            int64_t key = -1;
            if (src && pos < len) {
                const int64_t id = src[q * len + pos];
                if (tab) key = (id >= 0 && id < tab_len) ? tab[id] : -1;
                else key = id;
            }
            s_key[l * depth + pos] = key < 0 ? -1 : key;
        }
    }
    __syncthreads();
    // 2. ranks skip absent entries: contribution = contrib[list, present entries in front]
    for (int e = tid; e < n; e += kBlock) {
        const int l = e / depth, base = l * depth;
        int before = 0;
        for (int j = base; j < e; ++j) before += s_key[j] >= 0 ? 1 : 0;
        s_val[e] = s_key[e] >= 0 ? p.contrib[base + before] : 0.0;
    }
    __syncthreads();
    // 3. first entries sum their key's contributions in chain order, from 0.0 as Python does (0.0 + -0.0 is +0.0)
    for (int e = tid; e < n; e += kBlock) {
        const int64_t key = s_key[e];
        bool first = key >= 0;
        double sum = 0.0;
        if (first) {
            sum += s_val[e];
            for (int j = 0; j < n; ++j) {
                if (s_key[j] != key) continue;
                if (j < e) { first = false; break; }
                if (j > e) sum += s_val[j];
            }
        }
        s_score[e] = first ? sum : -1.0;
    }
    __syncthreads();
    // 4. slot by counting; the slots past the distinct keys are padding
    int distinct = 0;
    for (int j = 0; j < n; ++j) distinct += s_score[j] >= 0.0 ? 1 : 0;
    const int64_t out0 = q * p.k_out;
    for (int e = tid; e < n; e += kBlock) {
        const double sc = s_score[e];
        if (!(sc >= 0.0)) continue;
        int slot = 0;
        for (int j = 0; j < n; ++j) {
            const double sj = s_score[j];
            slot += (sj > sc || (sj == sc && j < e)) ? 1 : 0;
        }
        if (slot >= p.k_out) continue;
        const int l = e / depth;
        int64_t key = s_key[e];
        if (p.resolve) {
#pragma unroll
            for (int m = 0; m < RMU_RRF_MAX_LISTS; ++m)
                if (m == l) key = p.ids[m][q * p.len[m] + (e - l * depth)];
        }
        p.out_scores[out0 + slot] = sc;
        p.out_keys[out0 + slot] = key;
        p.out_src[out0 + slot] = p.resolve ? l : e;
    }
    for (int slot = distinct + tid; slot < p.k_out; slot += kBlock) {
        p.out_scores[out0 + slot] = -INFINITY;
        p.out_keys[out0 + slot] = -1;
        p.out_src[out0 + slot] = -1;
    }
}

// per-thread workspaces.  rmu_rrf_fuse given a caller stream and device buffers leaves its work in flight on them: `ev` marks its end and the
// thread's next call waits for it on the host before it touches them again (rare: every other form of the calls drains its stream)
struct Ctx {
    RmuDevBuf keys, contrib, out;
    RmuPinBuf pin{8192};       // the contribution table on its way in | the results on their way out
    hipEvent_t ev = nullptr;
    bool pending = false;
    int settle() {
        if (pending && hipEventSynchronize(ev) != hipSuccess) return RMU_E_HIP;
        pending = false;
        return RMU_OK;
    }
    void finished(hipStream_t s, bool drained) {
        if (drained) { pending = false; return; }
        if ((ev || hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess) && hipEventRecord(ev, s) == hipSuccess) pending = true;
        else { (void)hipGetLastError(); (void)hipStreamSynchronize(s); pending = false; }
    }
    // only what has an order: the work in flight ends, the event goes; the buffers free themselves behind this body
    ~Ctx() {
        if (rmu_runtime_down() || !ev) return;
        RMU_ENTRY();
        if (pending) (void)hipEventSynchronize(ev);
        (void)hipEventDestroy(ev);
    }
};
thread_local Ctx g_ctx;

// contributions of list l at [l * depth + rank - 1]; Python's  w / (rank + c)  with an int sum converted exactly
void fill_contrib(double* tab, const double* weights, const int* lens, int lists, int depth, int c) {
    for (int l = 0; l < lists; ++l)
        for (int r = 0; r < depth; ++r)
            tab[l * depth + r] = r < lens[l] ? weights[l] / (double)((int64_t)(r + 1) + (int64_t)c) : 0.0;
}
bool weights_ok(const double* w, int lists) {
    for (int l = 0; l < lists; ++l)
        if (!std::isfinite(w[l]) || !(w[l] >= 0.0)) return false;
    return true;
}
size_t out_bytes_of(int64_t nq, int k_out) { return (size_t)nq * k_out * (sizeof(double) + sizeof(int64_t) + sizeof(int32_t)); }

// (the workspaces are sized, the table is in pinned memory) table to the device, the kernel, and -- host outputs -- the results to pinned memory
int fuse_enqueue(Ctx& c, RrfLaunch& L, int64_t nq, bool out_host, hipStream_t s) {
    const size_t tab_bytes = (size_t)L.lists * L.depth * sizeof(double);
    RMU_HIP_TRY(hipMemcpyAsync(c.contrib.p, c.pin.p, tab_bytes, hipMemcpyHostToDevice, s));
    L.contrib = (const double*)c.contrib.p;
    if (out_host) {
        const size_t nk = (size_t)nq * L.k_out;
        L.out_scores = (double*)c.out.p;
        L.out_keys = (int64_t*)(L.out_scores + nk);
        L.out_src = (int32_t*)(L.out_keys + nk);
    }
    hipLaunchKernelGGL(rrf_fuse_kernel, dim3((unsigned)nq), dim3(kBlock), 0, s, L);
    RMU_HIP_TRY(hipGetLastError());
    if (out_host) RMU_HIP_TRY(hipMemcpyAsync(c.pin.p + kMaxEntries * sizeof(double), c.out.p, out_bytes_of(nq, L.k_out), hipMemcpyDeviceToHost, s));
    return RMU_OK;
}
void take_results(const Ctx& c, int64_t nq, int k_out, double* out_scores, int64_t* out_keys, int32_t* out_src) {
    const size_t nk = (size_t)nq * k_out;
    const char* src = c.pin.p + kMaxEntries * sizeof(double);
    memcpy(out_scores, src, nk * sizeof(double));
    memcpy(out_keys, src + nk * sizeof(double), nk * sizeof(int64_t));
    memcpy(out_src, src + nk * (sizeof(double) + sizeof(int64_t)), nk * sizeof(int32_t));
}

}  // namespace

extern "C" int rmu_rrf_fuse(const int64_t* keys, int lists, int64_t nq, int depth, const double* weights, int c, int k_out, unsigned flags,
                            double* out_scores, int64_t* out_keys, int32_t* out_src, uint64_t hip_stream) {
    RMU_ENTRY();
    if (!keys || !weights || !out_scores || !out_keys || !out_src) return rmu_fail(RMU_E_INVALID, "rmu_rrf_fuse: null pointer");
    if (lists < 1 || lists > RMU_RRF_MAX_LISTS) return rmu_fail(RMU_E_INVALID, "rmu_rrf_fuse: 1 <= lists <= RMU_RRF_MAX_LISTS (4)");
    if (depth < 1 || depth > RMU_MAX_K) return rmu_fail(RMU_E_INVALID, "rmu_rrf_fuse: 1 <= depth <= RMU_MAX_K (112)");
    if (k_out < 1 || k_out > lists * depth) return rmu_fail(RMU_E_INVALID, "rmu_rrf_fuse: 1 <= k_out <= lists * depth");
    if (nq < 1 || nq > 0x7FFFFFFFll) return rmu_fail(RMU_E_INVALID, "rmu_rrf_fuse: 1 <= nq <= 2^31 - 1");
    if (c < 0) return rmu_fail(RMU_E_INVALID, "rmu_rrf_fuse: c must be >= 0");
    if (!weights_ok(weights, lists)) return rmu_fail(RMU_E_INVALID, "rmu_rrf_fuse: every weight must be finite and >= 0");
    const bool in_dev = flags & RMU_F_Q_DEVICE, out_dev = flags & RMU_F_OUT_DEVICE;

    Ctx& x = g_ctx;
    if (x.settle() != RMU_OK) return rmu_fail(RMU_E_HIP, "rmu_rrf_fuse: waiting for the thread's previous call");
    hipStream_t s = nullptr;
    int rc = rmu_thread_stream_((hipStream_t)hip_stream, &s);
    if (rc) return rc;
    const size_t in_bytes = (size_t)lists * nq * depth * sizeof(int64_t);
    if (x.pin.ensure(kMaxEntries * sizeof(double) + (out_dev ? 0 : out_bytes_of(nq, k_out))) != RMU_OK)
        return rmu_fail(RMU_E_OOM, "rmu_rrf_fuse: pinned staging buffer");
    RMU_HIP_TRY(x.contrib.ensure(kMaxEntries * sizeof(double)));
    if (!in_dev) RMU_HIP_TRY(x.keys.ensure(in_bytes));
    if (!out_dev) RMU_HIP_TRY(x.out.ensure(out_bytes_of(nq, k_out)));

    RrfLaunch L{};
    const int64_t* dk = keys;
    if (!in_dev) {
        RMU_HIP_TRY(hipMemcpyAsync(x.keys.p, keys, in_bytes, hipMemcpyHostToDevice, s));
        dk = (const int64_t*)x.keys.p;
    }
    int lens[RMU_RRF_MAX_LISTS] = {0, 0, 0, 0};
    for (int l = 0; l < lists; ++l) {
        L.ids[l] = dk + (size_t)l * nq * depth;
        L.len[l] = lens[l] = depth;
    }
    L.lists = lists; L.depth = depth; L.k_out = k_out; L.resolve = 0;
    L.out_scores = out_scores; L.out_keys = out_keys; L.out_src = out_src;
    fill_contrib((double*)x.pin.p, weights, lens, lists, depth, c);
    rc = fuse_enqueue(x, L, nq, !out_dev, s);
    if (rc) { (void)hipStreamSynchronize(s); x.finished(s, true); rmu_thread_finished_(s, true); return rc; }
    const bool drained = !hip_stream || !out_dev || !in_dev;
    if (drained) {
        RMU_HIP_TRY(hipStreamSynchronize(s));
        if (!out_dev) take_results(x, nq, k_out, out_scores, out_keys, out_src);
    }
    x.finished(s, drained);
    rmu_thread_finished_(s, drained);
    return RMU_OK;
}

// ---- the one-call hybrid ---------------------------------------------------------------------------------------------------------------
struct rmu_hybrid {
    rmu_bm25_t* sparse = nullptr;      // borrowed
    rmu_index_t* dense = nullptr;      // borrowed
    // key tables: member m's id i -> key.  The host copy is the master (set_keys is host work); the device copy follows lazily: its first
    // d_len[m] entries are current, the rest is uploaded by the next search under the exclusive lock
    std::vector<int64_t> keys[2];
    int64_t* d_keys[2] = {nullptr, nullptr};
    size_t d_cap[2] = {0, 0};
    size_t d_len[2] = {0, 0};
    std::shared_mutex mu;
};

extern "C" int rmu_hybrid_create(rmu_hybrid_t** out, rmu_bm25_t* sparse, rmu_index_t* dense) {
    RMU_ENTRY();
    if (!out) return rmu_fail(RMU_E_INVALID, "rmu_hybrid_create: out is null");
    if (!sparse && !dense) return rmu_fail(RMU_E_INVALID, "rmu_hybrid_create: at least one member is needed");
    rmu_hybrid* h = new (std::nothrow) rmu_hybrid();
    if (!h) return rmu_fail(RMU_E_OOM, "rmu_hybrid_create: out of memory");
    h->sparse = sparse;
    h->dense = dense;
    *out = h;
    return RMU_OK;
}

extern "C" int rmu_hybrid_free(rmu_hybrid_t* h) {
    RMU_ENTRY();
    if (!h) return RMU_OK;
    {
        std::unique_lock<std::shared_mutex> lk(h->mu);      // searches end under the shared lock with their stream drained
        for (int m = 0; m < 2; ++m)
            if (h->d_keys[m]) (void)rmu_free(h->d_keys[m]);
    }
    delete h;
    return RMU_OK;
}

extern "C" int rmu_hybrid_set_keys(rmu_hybrid_t* h, int member, int64_t first, const int64_t* keys, int64_t n) {
    if (!h || (member != 0 && member != 1) || n < 0 || (n > 0 && !keys)) return rmu_fail(RMU_E_INVALID, "rmu_hybrid_set_keys: bad argument");
    std::unique_lock<std::shared_mutex> lk(h->mu);
    std::vector<int64_t>& tab = h->keys[member];
    if (first < 0 || (uint64_t)first > tab.size())
        return rmu_fail(RMU_E_INVALID, "rmu_hybrid_set_keys: first (" + std::to_string(first) + ") is beyond the table's length (" + std::to_string(tab.size()) + ")");
    for (int64_t i = 0; i < n; ++i)
        if (keys[i] < 0) return rmu_fail(RMU_E_INVALID, "rmu_hybrid_set_keys: a key is negative");
    try {
        tab.resize((size_t)(first + n));
    } catch (...) { return rmu_fail(RMU_E_OOM, "rmu_hybrid_set_keys: out of memory"); }
    if (n) memcpy(tab.data() + first, keys, (size_t)n * sizeof(int64_t));
    if (h->d_len[member] > (size_t)first) h->d_len[member] = (size_t)first;
    return RMU_OK;
}

// (exclusive lock held: no search of this handle is in flight) bring the device tables up to the host's; drains s
static int upload_tables(rmu_hybrid* h, hipStream_t s) {
    for (int m = 0; m < 2; ++m) {
        const size_t n = h->keys[m].size();
        if (h->d_len[m] == n) continue;
        if (n > h->d_cap[m]) {
            if (h->d_keys[m]) (void)rmu_free(h->d_keys[m]);
            h->d_keys[m] = nullptr; h->d_cap[m] = 0; h->d_len[m] = 0;
            const size_t cap = n + n / 4 + 1024;
            RMU_HIP_TRY(hipMalloc((void**)&h->d_keys[m], cap * sizeof(int64_t)));
            h->d_cap[m] = cap;
        }
        if (h->d_len[m] < n)
            RMU_HIP_TRY(hipMemcpyAsync(h->d_keys[m] + h->d_len[m], h->keys[m].data() + h->d_len[m], (n - h->d_len[m]) * sizeof(int64_t), hipMemcpyHostToDevice, s));
    }
    RMU_HIP_TRY(hipStreamSynchronize(s));          // (the host vectors are pageable)
    for (int m = 0; m < 2; ++m) h->d_len[m] = h->keys[m].size();
    return RMU_OK;
}

// every limit of the call, without touching HIP
static int hybrid_check(const rmu_hybrid* h, const void* q, int64_t nq, const char* blob, int64_t bytes, int k_sparse, int fetch_k, int k_dense,
                        const double* weights, int c, int k_out, const void* o1, const void* o2, const void* o3, const char* who) {
    const std::string w(who);
    if (!h || !q || !blob || !weights || !o1 || !o2 || !o3) return rmu_fail(RMU_E_INVALID, w + ": null argument");
    if (nq < 1 || nq > 65535 || bytes < nq) return rmu_fail(RMU_E_INVALID, w + ": 1 <= nq <= 65535 queries, each NUL-terminated");
    if (k_sparse < 1 || k_sparse > RMU_MAX_K) return rmu_fail(RMU_E_INVALID, w + ": 1 <= k_sparse <= RMU_MAX_K");
    if (fetch_k < 1 || fetch_k > 64 || k_dense < 1 || k_dense > fetch_k) return rmu_fail(RMU_E_INVALID, w + ": fetch_k in [1, 64], k_dense in [1, fetch_k]");
    if (k_out < 1 || k_out > k_sparse + k_dense) return rmu_fail(RMU_E_INVALID, w + ": 1 <= k_out <= k_sparse + k_dense");
    if (c < 0) return rmu_fail(RMU_E_INVALID, w + ": c must be >= 0");
    if (!weights_ok(weights, 2)) return rmu_fail(RMU_E_INVALID, w + ": every weight must be finite and >= 0");
    int64_t strings = 0;
    for (int64_t i = 0; i < bytes; ++i) strings += blob[i] == '\0';
    if (strings != nq || blob[bytes - 1] != '\0') return rmu_fail(RMU_E_INVALID, w + ": the blob does not hold exactly nq NUL-terminated strings");
    return RMU_OK;
}

// q: host, or (q_dev) device queries already on `user`; everything else as rmu_hybrid_search
static int hybrid_search(rmu_hybrid* h, const float* q, bool q_dev, int64_t nq, const char* blob, int64_t bytes, int k_sparse, int fetch_k, int k_dense,
                         double lambda_mult, const double* weights, int c, int k_out, double* out_scores, int64_t* out_ids, int32_t* out_member,
                         hipStream_t user, const char* who) {
    int rc = hybrid_check(h, q, nq, blob, bytes, k_sparse, fetch_k, k_dense, weights, c, k_out, out_scores, out_ids, out_member, who);
    if (rc) return rc;
    const std::string w(who);
    if (std::isnan(lambda_mult)) return rmu_fail(RMU_E_INVALID, w + ": lambda_mult is not a number");
    Ctx& x = g_ctx;
    const int depth = k_sparse > k_dense ? k_sparse : k_dense;
    const int lens[RMU_RRF_MAX_LISTS] = {k_sparse, k_dense, 0, 0};

    std::shared_lock<std::shared_mutex> lk(h->mu);
    // the members' records against the tables, before anything is enqueued (the members check again under their own locks)
    if (!h->sparse && !h->keys[0].empty()) return rmu_fail(RMU_E_INVALID, w + ": a sparse key table without a sparse member: out of step");
    if (!h->dense && !h->keys[1].empty()) return rmu_fail(RMU_E_INVALID, w + ": a dense key table without a dense member: out of step");
    if (h->sparse) {
        double docs = 0.0;
        if ((rc = rmu_bm25_stat(h->sparse, RMU_BM25_STAT_DOCS, &docs))) return rc;
        if ((int64_t)docs != (int64_t)h->keys[0].size())
            return rmu_fail(RMU_E_INVALID, w + ": the sparse key table (" + std::to_string(h->keys[0].size()) + " keys) and the BM25 index (" +
                                            std::to_string((int64_t)docs) + " documents) are out of step");
    }
    if (h->dense) {
        int64_t rows = 0;
        if ((rc = rmu_index_size(h->dense, &rows))) return rc;
        if (rows != (int64_t)h->keys[1].size())
            return rmu_fail(RMU_E_INVALID, w + ": the dense key table (" + std::to_string(h->keys[1].size()) + " keys) and the index (" + std::to_string(rows) +
                                            " rows) are out of step");
    }
    if (x.settle() != RMU_OK) return rmu_fail(RMU_E_HIP, w + ": waiting for the thread's previous call");
    hipStream_t s = nullptr;
    if ((rc = rmu_thread_stream_(user, &s))) return rc;
    while (h->d_len[0] != h->keys[0].size() || h->d_len[1] != h->keys[1].size()) {
        lk.unlock();
        {
            std::unique_lock<std::shared_mutex> wl(h->mu);
            if ((rc = upload_tables(h, s))) return rc;
        }
        lk.lock();
    }
    if (x.pin.ensure(kMaxEntries * sizeof(double) + out_bytes_of(nq, k_out)) != RMU_OK) return rmu_fail(RMU_E_OOM, w + ": pinned staging buffer");
    RMU_HIP_TRY(x.contrib.ensure(kMaxEntries * sizeof(double)));
    RMU_HIP_TRY(x.out.ensure(out_bytes_of(nq, k_out)));

    // the two members, one behind the other on s; their shared locks stay held until s is drained
    std::shared_lock<std::shared_mutex> lk_sparse, lk_dense;
    RrfLaunch L{};
    if (h->sparse) {
        bool empty = false;
        const int64_t* d_docs = nullptr;
        rc = rmu_bm25_search_enqueue_(h->sparse, blob, bytes, nq, k_sparse, (int64_t)h->keys[0].size(), s, lk_sparse, &d_docs, &empty);
        if (rc) return rc;                                      // (nothing of this call is in flight: the sparse member goes first)
        L.ids[0] = empty ? nullptr : d_docs;
    }
    if (h->dense) {
        const int64_t* d_rows = nullptr;
        rc = rmu_index_search_mmr_enqueue_(h->dense, q, q_dev, nq, fetch_k, k_dense, lambda_mult, (int64_t)h->keys[1].size(), s, who, lk_dense, &d_rows);
        if (rc) { (void)hipStreamSynchronize(s); rmu_thread_finished_(s, true); return rc; }
        L.ids[1] = d_rows;
    }
    for (int m = 0; m < 2; ++m) {
        L.table[m] = h->d_keys[m];
        L.table_len[m] = (int64_t)h->d_len[m];
        L.len[m] = lens[m];
        if (!L.table[m]) L.ids[m] = nullptr;                    // an empty table: the member has no records
    }
    L.lists = 2; L.depth = depth; L.k_out = k_out; L.resolve = 1;
    fill_contrib((double*)x.pin.p, weights, lens, 2, depth, c);
    rc = fuse_enqueue(x, L, nq, true, s);
    const hipError_t es = hipStreamSynchronize(s);
    x.finished(s, true);
    rmu_thread_finished_(s, true);
    if (rc) return rc;
    RMU_HIP_TRY(es);
    take_results(x, nq, k_out, out_scores, out_ids, out_member);
    return RMU_OK;
}

extern "C" int rmu_hybrid_search(rmu_hybrid_t* h, const float* q, int64_t nq, const char* query_blob, int64_t bytes, int k_sparse, int fetch_k,
                                 int k_dense, double lambda_mult, const double* weights, int c, int k_out, double* out_scores, int64_t* out_ids,
                                 int32_t* out_member, uint64_t hip_stream) {
    RMU_ENTRY();
    return hybrid_search(h, q, false, nq, query_blob, bytes, k_sparse, fetch_k, k_dense, lambda_mult, weights, c, k_out, out_scores, out_ids, out_member,
                         (hipStream_t)hip_stream, "rmu_hybrid_search");
}

// bert.hip (rmu_bert_search_hybrid): the limits alone, in front of the forward; then the same call over DEVICE queries on the encoder's stream
extern "C" int rmu_hybrid_check_(rmu_hybrid_t* h, rmu_index_t** dense, int64_t nq, const char* query_blob, int64_t bytes, int k_sparse, int fetch_k,
                                 int k_dense, const double* weights, int c, int k_out, double* out_scores, int64_t* out_ids, int32_t* out_member) {
    const int rc = hybrid_check(h, h, nq, query_blob, bytes, k_sparse, fetch_k, k_dense, weights, c, k_out, out_scores, out_ids, out_member,
                                "rmu_bert_search_hybrid");
    if (rc) return rc;
    *dense = h->dense;
    return RMU_OK;
}
extern "C" int rmu_hybrid_search_dev_(rmu_hybrid_t* h, const float* q_dev, int64_t nq, const char* query_blob, int64_t bytes, int k_sparse, int fetch_k,
                                      int k_dense, double lambda_mult, const double* weights, int c, int k_out, double* out_scores, int64_t* out_ids,
                                      int32_t* out_member, void* hip_stream) {
    RMU_ENTRY();
    if (!hip_stream) return rmu_fail(RMU_E_INVALID, "rmu_bert_search_hybrid: null stream");
    return hybrid_search(h, q_dev, true, nq, query_blob, bytes, k_sparse, fetch_k, k_dense, lambda_mult, weights, c, k_out, out_scores, out_ids,
                         out_member, (hipStream_t)hip_stream, "rmu_bert_search_hybrid");
}
